"""GPU tests (-m gpu) of the spatial null (include/dsabf.h: bf_null_solve_device, bf_null_weights_device; docs/NULLING.md).  The
reference is tests/support/null_oracle.py -- numpy float64 in the contract's one summation order -- and every comparison of vectors,
eigenvalues, info, weights and scales is np.array_equal on the raw bits: outputs are filled with a sentinel first (a NaN payload for
the float64 arrays, 0x7F bytes for info and weights) and compared whole.

Every test is ONE function that loops over its cases, as tests/test_gpu_cal.py does."""
import os
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

SUPPORT = os.path.join(ROOT, "tests", "support")
sys.path.insert(0, SUPPORT)
import cal_oracle  # noqa: E402
import corr_oracle  # noqa: E402
import null_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

BF_ERR_INVALID = -1
NAN_BITS = 0x7FF8DEADBEEF0001        # a quiet NaN with a payload no arithmetic produces
INFO_FILL = 0x7F7F7F7F


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need a GPU"
    return t


@pytest.fixture(scope="module")
def bfmod():
    import dsabeamformer_amd as m

    return m


def _cfg(bfmod, n_ant, n_pol=1, n_freq=1, n_beams=8, **over):
    kw = dict(n_ant=n_ant, n_pol=n_pol, n_avg=1, n_beams=n_beams, n_freq=n_freq, n_out_per_gemm=2, n_gemms_per_block=4, n_blocks_on_gpu=2,
              n_streams=4)
    kw.update(over)
    return bfmod.debug_config(**kw)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _outputs(torch, cfg, n_null):
    return (torch.full((cfg.n_freq, n_null, cfg.n_ant, 2), NAN_BITS, dtype=torch.int64, device="cuda"),
            torch.full((cfg.n_freq, n_null + 1), NAN_BITS, dtype=torch.int64, device="cuda"),
            torch.full((cfg.n_freq, 1 + 2 * n_null), INFO_FILL, dtype=torch.int32, device="cuda"))


def _solve(torch, bf, vis, flags=None, n_null=1, **opt):
    """One solve through the Python API: (bits of the vectors, bits of the eigenvalues, info)."""
    d_v, d_e, d_i = _outputs(torch, bf.cfg, n_null)
    d_vis, d_f = _dev(torch, vis), _dev(torch, flags)
    bf.null_solve(d_vis, d_v, d_e, d_i, flags=d_f, n_null=n_null, **opt)
    torch.cuda.synchronize()
    return d_v.cpu().numpy(), d_e.cpu().numpy(), d_i.cpu().numpy()


def _same(got, want, tag):
    (gv, ge, gi), (wv, we, wi) = got, want
    assert np.array_equal(gi, wi), (tag, gi.tolist(), wi.tolist())
    assert np.array_equal(ge, _bits(we)), (tag, ge.view(np.float64).tolist(), we.tolist())
    bad = np.argwhere(gv != _bits(wv))
    assert bad.size == 0, (tag, len(bad), bad[:4], gv.view(np.float64)[tuple(bad[0])], wv[tuple(bad[0])])


def _signatures(rng, n_int, n_ant):
    return np.exp(2j * np.pi * rng.uniform(size=(n_int, n_ant)))


def _field(rng, n_ant, n_freq, n_pol, n_int, noise):
    """n_int interferers of powers 3000 and 1000 in every channel but channel 1, which holds the noise alone."""
    pw = np.zeros((max(n_int, 1), n_freq))
    for i in range(n_int):
        pw[i] = 3000.0 / (1 + 2 * i)
    if n_freq > 1:
        pw[:, 1] = 0.0
    return null_oracle.exact_vis(_signatures(rng, max(n_int, 1), n_ant), pw, n_ant, n_freq, n_pol, noise=noise, seed=int(rng.integers(1 << 30)))


def _flags(rng, vis, n_ant):
    """Antennas 0 and n - 2 flagged, and garbage wherever they take part in `vis`."""
    flags = np.zeros(n_ant, np.uint8)
    flags[[0, n_ant - 2]] = 1
    for a in (0, n_ant - 2):
        idx = [cal_oracle.bl(max(a, b), min(a, b)) for b in range(n_ant)]
        vis[:, :, idx] = rng.integers(-2 ** 40, 2 ** 40, size=vis.shape[:2] + (n_ant, 2))
    return flags


# (n_ant, n_freq, n_pol, pol, n_null, interferers, flags, path, noise): path "auto" is what the library picks (LDS-resident up to 64
# antennas, streamed above), "streamed" forces the re-reading path where the resident one would run.  noise 0 leaves exact low-rank
# matrices: all zeros without an interferer, so the early end (status 2) occurs; with noise the surplus vectors are found and not used.
COUNT_CASES = [(4, 1, 1, -1, 1, 0, False, "auto", 0), (4, 3, 2, 1, 2, 1, True, "auto", 20), (4, 3, 2, -1, 4, 2, False, "streamed", 20),
               (20, 3, 2, -1, 2, 1, True, "auto", 20), (20, 1, 1, -1, 4, 2, False, "streamed", 0),
               (64, 3, 2, 1, 1, 0, False, "auto", 20), (64, 3, 2, -1, 2, 2, True, "auto", 20), (64, 1, 2, -1, 4, 1, True, "streamed", 20),
               (68, 3, 2, -1, 2, 1, True, "auto", 20),
               (132, 3, 2, 1, 4, 2, True, "auto", 20), (132, 1, 1, -1, 1, 1, False, "auto", 20),
               (256, 1, 1, -1, 1, 0, False, "auto", 20), (256, 3, 2, -1, 2, 1, True, "auto", 20), (256, 3, 2, 1, 4, 2, False, "auto", 20),
               (256, 1, 2, -1, 2, 2, True, "auto", 0)]


def test_every_antenna_count_to_the_bit(torch, bfmod):
    """Antenna counts 4, 20, 64, 68, 132, 256; 1 and 3 channels (channel 1 of three is interferer-free); n_null 1, 2, 4 against 0, 1, 2
    interferers; 1 and 2 polarisations with pol -1 and 1; no flags or {0, n - 2} flagged with garbage in the flagged rows; both storage
    paths at 64 antennas.  Vectors, eigenvalues and info whole, to the bit."""
    for idx, values in ((0, (4, 20, 64, 68, 132, 256)), (1, (1, 3)), (2, (1, 2)), (3, (-1, 1)), (4, (1, 2, 4)), (5, (0, 1, 2)), (6, (False, True))):
        assert {c[idx] for c in COUNT_CASES} == set(values), idx
    assert {(c[0], c[7]) for c in COUNT_CASES} >= {(64, "auto"), (64, "streamed"), (68, "auto")}
    rng = np.random.default_rng(20261019)
    t0 = time.perf_counter()
    seen_status, unused = set(), 0
    for case in COUNT_CASES:
        n_ant, n_freq, n_pol, pol, n_null, n_int, flagged, path, noise = case
        cfg = _cfg(bfmod, n_ant, n_pol, n_freq)
        vis = _field(rng, n_ant, n_freq, n_pol, n_int, noise)
        flags = _flags(rng, vis, n_ant) if flagged else None
        want = null_oracle.solve(vis, n_ant, flags, n_null=n_null, pol=pol)
        bf = bfmod.Beamformer(cfg)
        assert bf.null_vec_entries(n_null) * 2 == want[0].size
        if path == "streamed":
            bf.set_switch("null_resident", 0)
        got = _solve(torch, bf, vis, flags, n_null, pol=pol)
        bf.close()
        _same(got, want, case)
        wv, we, wi = want
        assert np.isfinite(wv).all() and np.isfinite(we).all()
        seen_status |= set(wi[:, 2::2].ravel().tolist())
        unused += int((wi[:, 0] < n_null).sum())
        for f in range(n_freq):
            assert not wv[f, wi[f, 0]:].any()                                # unused vectors: exact zeros
            if noise and not (n_freq > 1 and f == 1):                          # (four antennas cannot lift the weaker interferer 4 x above the rest)
                assert wi[f, 0] == min(n_int, n_null, 1 if n_ant == 4 else 2), (case, f, wi[f].tolist(), we[f].tolist())
            if noise and n_freq > 1 and f == 1:
                assert wi[f, 0] == 0, (case, wi[f].tolist(), we[f].tolist())
        if flagged:
            assert not wv[:, :, [0, n_ant - 2]].any()
    assert seen_status == {0, 1, 2} and unused > 0, (seen_status, unused)
    print("null_solve_kernel: %d cases, %.1f s" % (len(COUNT_CASES), time.perf_counter() - t0))


def _dft(n_ant, k):
    return np.exp(2j * np.pi * k * np.arange(n_ant) / n_ant)


def test_iteration_control_and_degenerates(torch, bfmod):
    """max_iter 1 and 3 (status 0 unless the distance is already below tol); a huge tol stops at the first multiplication; tol 0; two
    interferers of equal power and orthogonal signatures, which the power iteration cannot separate in 200 multiplications: status 0 and
    both vectors used; all-zero visibilities; one unflagged antenna; m <= n_null.  Zeros, never NaN, and the oracle's bits."""
    rng = np.random.default_rng(11)
    n_ant = 20
    cfg = _cfg(bfmod, n_ant, 2, 3)
    vis = _field(rng, n_ant, 3, 2, 2, 20)
    bf = bfmod.Beamformer(cfg)
    for opt, expect in ((dict(max_iter=1), (1, 0)), (dict(max_iter=3), (3, 0)), (dict(tol=1e3), (1, 1)), (dict(tol=0.0, max_iter=5), None),
                        (dict(min_ratio=0.0), None), (dict(min_ratio=1e9), None)):
        want = null_oracle.solve(vis, n_ant, n_null=2, **opt)
        _same(_solve(torch, bf, vis, None, 2, **opt), want, opt)
        if expect:
            assert want[2][0, 1:3].tolist() == list(expect), (opt, want[2].tolist())
        if "min_ratio" in opt:
            assert np.all(want[2][:, 0] == (2 if opt["min_ratio"] == 0 else 0)), want[2].tolist()
    one = np.ones(n_ant, np.uint8)
    one[3] = 0
    two = np.ones(n_ant, np.uint8)
    two[[3, 7]] = 0
    for name, v, flags, n_null in (("zeros", np.zeros_like(vis), None, 2), ("one antenna", vis, one, 1), ("m <= n_null", vis, two, 4)):
        want = null_oracle.solve(v, n_ant, flags, n_null=n_null)
        got = _solve(torch, bf, v, flags, n_null)
        _same(got, want, name)
        assert np.isfinite(got[0].view(np.float64)).all() and np.isfinite(got[1].view(np.float64)).all(), name
        if name == "zeros":
            assert not want[0].any() and np.all(want[2][:, 2::2] == 2) and np.all(want[2][:, 0] == 0)
        if name == "one antenna":
            assert not want[0].any() and np.all(want[2][:, 0] == 0)
        if name == "m <= n_null":
            assert np.all(want[2][:, 0] <= 1)
    bf.close()
    n_ant = 64
    sig = np.stack([_dft(n_ant, 3), _dft(n_ant, 17)])
    vis = null_oracle.exact_vis(sig, [[2000.0], [2000.0]], n_ant, 1, 2, noise=20, seed=5)
    want = null_oracle.solve(vis, n_ant, n_null=2)
    assert want[2][0].tolist()[:3] == [2, 200, 0], want[2].tolist()
    bf = bfmod.Beamformer(_cfg(bfmod, n_ant, 2, 1))
    _same(_solve(torch, bf, vis, None, 2), want, "equal powers")
    bf.close()


# (n_ant, n_beams)
WEIGHT_CASES = [(4, 4), (4, 8), (68, 60), (256, 8), (64, 256), (4, 260)]


def _weights(rng, n_freq, n_ant, n_beams):
    w = rng.integers(-127, 128, size=(n_freq, n_ant, n_beams, 2), dtype=np.int8)
    w[:, :, 0] = (127, 0)                                                    # +-127 on the axes: SCALED and CLIP differ
    w[:, :, 1] = (0, -127)
    w[1, :, 2] = (-128, -128)                                                # channel 1 is copied: whatever the bytes
    return w


def test_projected_weights_to_the_bit(torch, bfmod):
    """Beams 4, 8, 60, 256 (and 260: a second column per thread), antennas 4, 68, 256, both modes, with and without flags, weights with
    +-127 on the axes; three channels with 2, 0 and 1 used vectors: channel 1 comes back byte for byte.  In place; d_scale checked, and
    NULL."""
    rng = np.random.default_rng(23)
    t0 = time.perf_counter()
    assert {c[0] for c in WEIGHT_CASES} == {4, 68, 256, 64} and {c[1] for c in WEIGHT_CASES} >= {4, 8, 60, 256}
    differ = 0
    for n_ant, n_beams in WEIGHT_CASES:
        n_freq, n_null = 3, 2
        sig = _signatures(rng, 2, n_ant)
        vis = null_oracle.exact_vis(sig, [[3000.0, 0.0, 3000.0], [1500.0, 0.0, 0.0]], n_ant, n_freq, 1, noise=20, seed=n_ant + n_beams)
        w = _weights(rng, n_freq, n_ant, n_beams)
        bf = bfmod.Beamformer(_cfg(bfmod, n_ant, 1, n_freq, n_beams=n_beams))
        d_w = _dev(torch, w)
        for flagged in (False, True):
            v = vis.copy()
            flags = _flags(rng, v, n_ant) if flagged and n_ant > 4 else (np.array([0, 0, 1, 0], np.uint8) if flagged else None)
            vecs, eig, info = null_oracle.solve(v, n_ant, flags, n_null=n_null)
            assert info[:, 0].tolist() == [2 if n_ant > 4 else 1, 0, 1], (n_ant, flagged, info.tolist(), eig.tolist())
            d_vecs, d_info, d_f = _dev(torch, vecs), _dev(torch, info), _dev(torch, flags)
            outs = {}
            for mode, code in (("scaled", null_oracle.SCALED), ("clip", null_oracle.CLIP)):
                want_w, want_k = null_oracle.project(w, vecs, info, flags, code)
                d_out = torch.full(w.shape, 0x7F, dtype=torch.int8, device="cuda")
                d_k = torch.full((n_freq,), NAN_BITS, dtype=torch.int64, device="cuda")
                bf.null_weights(d_w, d_vecs, d_info, d_out, n_null, flags=d_f, mode=mode, scale=d_k)
                torch.cuda.synchronize()
                got = d_out.cpu().numpy()
                bad = np.argwhere(got != want_w)
                assert bad.size == 0, (n_ant, n_beams, mode, flagged, len(bad), bad[:4], got[tuple(bad[0])], want_w[tuple(bad[0])])
                assert np.array_equal(d_k.cpu().numpy(), _bits(want_k)), (mode, d_k.cpu().numpy().view(np.float64), want_k)
                assert want_k[1] == 1.0 and (mode == "scaled" or np.all(want_k == 1.0))
                live = np.ones(n_ant, bool) if flags is None else flags == 0
                assert np.array_equal(got[1][live], w[1][live]) and not got[:, ~live].any()   # channel 1: the bytes, -128 included
                assert got[[0, 2]].min() >= -127
                outs[mode] = got
                d_out2 = torch.full(w.shape, 0x7F, dtype=torch.int8, device="cuda")           # d_scale NULL
                bf.null_weights(d_w, d_vecs, d_info, d_out2, n_null, flags=d_f, mode=mode)
                d_same = d_w.clone()                                                          # in place
                bf.null_weights(d_same, d_vecs, d_info, d_same, n_null, flags=d_f, mode=mode)
                torch.cuda.synchronize()
                assert np.array_equal(d_out2.cpu().numpy(), want_w) and np.array_equal(d_same.cpu().numpy(), want_w)
            differ += int(not np.array_equal(outs["scaled"], outs["clip"]))
        bf.close()
    assert differ >= len(WEIGHT_CASES), differ
    print("null_apply_kernel: %d cases, %.1f s" % (len(WEIGHT_CASES), time.perf_counter() - t0))


def test_invalid_arguments_launch_nothing(torch, bfmod):
    """260 antennas, n_null 0 and 5, max_iter 0, tol or min_ratio negative or NaN, pol out of range, NULL and misaligned pointers, an
    unknown mode: BF_ERR_INVALID each, and the sentinels stay intact."""
    rng = np.random.default_rng(17)
    n_ant, n_freq = 8, 3
    cfg = _cfg(bfmod, n_ant, 2, n_freq)
    vis = _field(rng, n_ant, n_freq, 2, 1, 20)
    bf = bfmod.Beamformer(cfg)
    d_vis = _dev(torch, vis)
    d_v, d_e, d_i = _outputs(torch, cfg, 4)
    d_w = torch.full((n_freq, n_ant, 8, 2), 0x7F, dtype=torch.int8, device="cuda")
    d_u = torch.zeros((n_freq, 1, n_ant, 2), dtype=torch.float64, device="cuda")
    d_n = torch.ones((n_freq, 3), dtype=torch.int32, device="cuda")
    d_k = torch.full((n_freq,), NAN_BITS, dtype=torch.int64, device="cuda")
    lib, h = bf._lib, bf._h
    from dsabeamformer_amd._lib import BfNullOptions

    opt = BfNullOptions(4.0, 1e-6, 1, 200, -1)
    import ctypes as C

    bad = [lambda: bf.null_solve(d_vis, d_v, d_e, d_i, n_null=0), lambda: bf.null_solve(d_vis, d_v, d_e, d_i, n_null=5),
           lambda: bf.null_solve(d_vis, d_v, d_e, d_i, max_iter=0), lambda: bf.null_solve(d_vis, d_v, d_e, d_i, tol=-1e-3),
           lambda: bf.null_solve(d_vis, d_v, d_e, d_i, tol=float("nan")), lambda: bf.null_solve(d_vis, d_v, d_e, d_i, min_ratio=-1.0),
           lambda: bf.null_solve(d_vis, d_v, d_e, d_i, min_ratio=float("nan")), lambda: bf.null_solve(d_vis, d_v, d_e, d_i, pol=2),
           lambda: bf.null_solve(d_vis, d_v, d_e, d_i, pol=-2),
           lambda: bf.null_solve(None, d_v, d_e, d_i), lambda: bf.null_solve(d_vis, None, d_e, d_i), lambda: bf.null_solve(d_vis, d_v, None, d_i),
           lambda: bf.null_solve(d_vis, d_v, d_e, None),
           lambda: lib.bf_null_solve_device(h, d_vis.data_ptr(), None, None, d_v.data_ptr(), d_e.data_ptr(), d_i.data_ptr(), None),
           lambda: lib.bf_null_solve_device(h, d_vis.data_ptr() + 8, None, C.byref(opt), d_v.data_ptr(), d_e.data_ptr(), d_i.data_ptr(), None),
           lambda: lib.bf_null_solve_device(h, d_vis.data_ptr(), None, C.byref(opt), d_v.data_ptr() + 8, d_e.data_ptr(), d_i.data_ptr(), None),
           lambda: lib.bf_null_solve_device(h, d_vis.data_ptr(), None, C.byref(opt), d_v.data_ptr(), d_e.data_ptr() + 4, d_i.data_ptr(), None),
           lambda: lib.bf_null_solve_device(h, d_vis.data_ptr(), None, C.byref(opt), d_v.data_ptr(), d_e.data_ptr(), d_i.data_ptr() + 2, None),
           lambda: lib.bf_null_weights_device(h, d_w.data_ptr(), d_u.data_ptr(), d_n.data_ptr(), 1, None, 2, d_w.data_ptr(), None, None),
           lambda: lib.bf_null_weights_device(h, d_w.data_ptr(), d_u.data_ptr(), d_n.data_ptr(), 0, None, 0, d_w.data_ptr(), None, None),
           lambda: lib.bf_null_weights_device(h, d_w.data_ptr(), d_u.data_ptr(), d_n.data_ptr(), 5, None, 0, d_w.data_ptr(), None, None),
           lambda: lib.bf_null_weights_device(h, d_w.data_ptr() + 2, d_u.data_ptr(), d_n.data_ptr(), 1, None, 0, d_w.data_ptr(), None, None),
           lambda: lib.bf_null_weights_device(h, d_w.data_ptr(), d_u.data_ptr() + 8, d_n.data_ptr(), 1, None, 0, d_w.data_ptr(), None, None),
           lambda: lib.bf_null_weights_device(h, d_w.data_ptr(), d_u.data_ptr(), d_n.data_ptr(), 1, None, 0, d_w.data_ptr() + 1, None, None),
           lambda: lib.bf_null_weights_device(h, d_w.data_ptr(), d_u.data_ptr(), d_n.data_ptr(), 1, None, 0, d_w.data_ptr(), d_k.data_ptr() + 4, None),
           lambda: bf.null_weights(None, d_u, d_n, d_w, 1), lambda: bf.null_weights(d_w, None, d_n, d_w, 1),
           lambda: bf.null_weights(d_w, d_u, None, d_w, 1), lambda: bf.null_weights(d_w, d_u, d_n, None, 1)]
    for i, call in enumerate(bad):
        try:
            rc = call()
        except bfmod.DsabfError as e:
            rc = e.code
        assert rc == BF_ERR_INVALID, i
    with pytest.raises(ValueError):
        bf.null_weights(d_w, d_u, d_n, d_w, 1, mode="both")
    bf.close()
    wide = bfmod.Beamformer(_cfg(bfmod, 260, 1, 1))
    d_wvis = torch.zeros((1, 1, 260 * 261 // 2, 2), dtype=torch.int64, device="cuda")
    d_wv, d_we, d_wi = _outputs(torch, wide.cfg, 1)
    d_ww = torch.full((1, 260, 8, 2), 0x7F, dtype=torch.int8, device="cuda")
    d_wu = torch.zeros((1, 1, 260, 2), dtype=torch.float64, device="cuda")
    d_wn = torch.ones((1, 3), dtype=torch.int32, device="cuda")
    for call in (lambda: wide.null_solve(d_wvis, d_wv, d_we, d_wi), lambda: wide.null_weights(d_ww, d_wu, d_wn, d_ww, 1)):
        with pytest.raises(bfmod.DsabfError, match="256") as e:
            call()
        assert e.value.code == BF_ERR_INVALID
    wide.close()
    torch.cuda.synchronize()
    for t, fill in ((d_v, NAN_BITS), (d_e, NAN_BITS), (d_i, INFO_FILL), (d_w, 0x7F), (d_k, NAN_BITS), (d_wv, NAN_BITS), (d_we, NAN_BITS),
                    (d_wi, INFO_FILL), (d_ww, 0x7F)):
        assert torch.all(t == fill).item()


def test_two_streams_without_synchronisation(torch, bfmod):
    """Two solves of different inputs into separate outputs on two streams, no synchronisation in between (the solver keeps nothing in
    the handle); then a solve queued on the stream of the bf_correlate_device that produces its input."""
    rng = np.random.default_rng(19)
    n_ant = 64
    cfg = _cfg(bfmod, n_ant, 2, 3, n_avg=4, n_out_per_gemm=8)
    bf = bfmod.Beamformer(cfg)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    fields = [_field(rng, n_ant, 3, 2, 2, 20) for _ in range(2)]
    d_vis = [_dev(torch, v) for v in fields]
    outs = [_outputs(torch, cfg, 2) for _ in range(2)]
    torch.cuda.synchronize()
    for k in range(2):
        bf.null_solve(d_vis[k], *outs[k], n_null=2, stream=streams[k].cuda_stream)
    torch.cuda.synchronize()
    for k in range(2):
        _same(tuple(o.cpu().numpy() for o in outs[k]), null_oracle.solve(fields[k], n_ant, n_null=2), k)
    assert not np.array_equal(outs[0][0].cpu().numpy(), outs[1][0].cpu().numpy())
    # correlate -> solve on one stream: random voltages are noise, so the iterations run out; the bits still match
    n_units = 4
    packed = rng.integers(0, 256, size=(n_units, 3, cfg.n_out_per_gemm * 2 * cfg.n_avg, n_ant), dtype=np.uint8)
    d_in = torch.from_numpy(packed).cuda()
    d_v = torch.full((3, 2, corr_oracle.n_baselines(n_ant), 2), -1, dtype=torch.int64, device="cuda")
    out = _outputs(torch, cfg, 1)
    torch.cuda.synchronize()
    s = streams[0].cuda_stream
    bf.correlate(d_in, n_units, d_v, stream=s)
    bf.null_solve(d_v, *out, max_iter=20, stream=s)
    torch.cuda.synchronize()
    vis = corr_oracle.visibilities(packed, 2)
    assert np.array_equal(d_v.cpu().numpy(), vis)
    _same(tuple(o.cpu().numpy() for o in out), null_oracle.solve(vis, n_ant, max_iter=20), "behind the correlator")
    bf.close()


N_ANT, N_FREQ, N_BEAMS, N_OUT, N_AVG, N_UNITS = 64, 2, 16, 8, 16, 32


def interferer_scene(seed=20261019):
    """The end-to-end scene, on the CPU: 64 antennas, 2 channels, 16 beams, 2 polarisations, 4096 columns per polarisation.  One
    interferer (unit-modulus signature) at amplitude 2 against unit noise in channel 0 only; random unit-modulus steering weights.
    -> dict(packed, rfi_only, w)."""
    assert N_UNITS * N_OUT * N_AVG == 4096
    rng = np.random.default_rng(seed)
    sig = _signatures(rng, 1, N_ANT)
    packed, rfi_only = null_oracle.scene(seed + 1, N_ANT, N_FREQ, N_UNITS, N_OUT * 2 * N_AVG, sig, [[2.0, 0.0]], noise=1.0)
    ph = 2 * np.pi * rng.uniform(size=(N_FREQ, N_ANT, N_BEAMS))
    w = np.stack([np.rint(127 * np.cos(ph)), np.rint(127 * np.sin(ph))], axis=-1).astype(np.int8)
    return dict(packed=packed, rfi_only=rfi_only, w=w, rng=rng)


def exact_power(packed, w):
    """sum over time of |sum_a v_a w_a|^2 per (channel, beam) in exact integers, as float64 (the detect stage's 1 / 127^2 left out)."""
    vr, vi = corr_oracle.RE[packed].astype(np.int64), corr_oracle.IM[packed].astype(np.int64)     # [u][f][t][a]
    wr, wi = w[..., 0].astype(np.int64), w[..., 1].astype(np.int64)                               # [f][a][b]
    re = np.einsum("ufta,fab->uftb", vr, wr) - np.einsum("ufta,fab->uftb", vi, wi)
    im = np.einsum("ufta,fab->uftb", vr, wi) + np.einsum("ufta,fab->uftb", vi, wr)
    return (re * re + im * im).sum(axis=(0, 2)).astype(np.float64)


def scene_oracle(sc):
    """correlate -> solve -> project (SCALED) on the CPU, and the test source: signature s with u_0^H s = 0 in channel 0, its matched
    weights in beam 0 of channel 0, its 4-bit voltages."""
    vis = corr_oracle.visibilities(sc["packed"], 2)
    vecs, eig, info = null_oracle.solve(vis, N_ANT)
    u = vecs[0, 0, :, 0] + 1j * vecs[0, 0, :, 1]
    s = np.exp(2j * np.pi * sc["rng"].uniform(size=N_ANT))
    s = s - u * np.vdot(u, s)                                                # u^H s = 0
    s = s / np.abs(s).max()
    w = sc["w"].copy()
    w[0, :, 0, 0], w[0, :, 0, 1] = np.rint(127 * s.real), np.rint(-127 * s.imag)   # w = 127 conj(s): the beam aimed at the source
    x = (sc["rng"].standard_normal((N_UNITS, 1, N_OUT * 2 * N_AVG)) + 1j * sc["rng"].standard_normal((N_UNITS, 1, N_OUT * 2 * N_AVG))) / np.sqrt(2)
    src = null_oracle.pack(3 * x[..., None] * s)                             # [unit][1][time][ant]
    src = np.concatenate([src, np.zeros_like(src)], axis=1)                  # channel 1: silence
    w_null, k, w_f = null_oracle.project(w, vecs, info, None, null_oracle.SCALED, return_float=True)
    return dict(vis=vis, vecs=vecs, eig=eig, info=info, w=w, w_null=w_null, k=k, w_f=w_f, src=src, s=s)


def test_an_interferer_is_nulled_and_the_sky_is_kept(torch, bfmod):
    """correlate -> solve -> project (BF_NULL_SCALED) -> bf_set_weights_device -> beamform.  (a) every device result equals the oracles
    to the bit; (b) the interferer-only block's detected power, summed over the beams of channel 0, is at most 1 / 20 of its value with
    the original weights (the oracle gives 0.0276 for this seed: the interferer's own 4-bit quantisation noise is not spatially coherent
    and stays); (c) channel 1's weights are byte-identical; (d) beam 0, aimed at a source whose signature is orthogonal to u_0, keeps it:
    the device power equals that of the oracle's unquantised k_f w' within the requantisation bound -- each weight moves by at most
    sqrt(0.5), so each beam sample by at most E_t = sqrt(0.5) sum_a |v_a|, and the power by sum_t (2 |y_t| E_t + E_t^2) -- plus the detect
    stage's 2 n_ipo 2^-24; and it is within 5 % of k_f^2 times the power with the original weights (the int8 rounding of the matched
    weights leaves |u^T w| <= sqrt(n / 2), which moves a sample by at most sqrt(32) |v| against |y| = 127 |s| |v|, |s| > 4: under 1.2 %
    in amplitude, and the requantisation under 1 %)."""
    sc = interferer_scene()
    orc = scene_oracle(sc)
    cfg = _cfg(bfmod, N_ANT, 2, N_FREQ, n_beams=N_BEAMS, n_avg=N_AVG, n_out_per_gemm=N_OUT, n_gemms_per_block=N_UNITS)
    n_ipo = 2 * N_AVG
    bf = bfmod.Beamformer(cfg)
    d_in, d_rfi, d_src, d_w_in = (torch.from_numpy(orc[k] if k in orc else sc[k]).cuda() for k in ("packed", "rfi_only", "src", "w"))
    d_vis = torch.full((N_FREQ, 2, corr_oracle.n_baselines(N_ANT), 2), -1, dtype=torch.int64, device="cuda")
    d_v, d_e, d_i = _outputs(torch, cfg, 1)
    d_w = torch.full(orc["w"].shape, 0x7F, dtype=torch.int8, device="cuda")
    d_k = torch.full((N_FREQ,), NAN_BITS, dtype=torch.int64, device="cuda")
    bf.correlate(d_in, N_UNITS, d_vis)
    bf.null_solve(d_vis, d_v, d_e, d_i)
    bf.null_weights(d_w_in, d_v, d_i, d_w, 1, scale=d_k)
    torch.cuda.synchronize()
    assert np.array_equal(d_vis.cpu().numpy(), orc["vis"])
    _same((d_v.cpu().numpy(), d_e.cpu().numpy(), d_i.cpu().numpy()), (orc["vecs"], orc["eig"], orc["info"]), "scene")
    assert orc["info"][:, 0].tolist() == [1, 0] and orc["info"][0, 2] == 1, orc["info"].tolist()
    assert np.array_equal(d_w.cpu().numpy(), orc["w_null"]) and np.array_equal(d_k.cpu().numpy(), _bits(orc["k"]))
    assert np.array_equal(d_w.cpu().numpy()[1], orc["w"][1]) and orc["k"][1] == 1.0 and orc["k"][0] <= 1.0          # (c)

    def power(d_weights, d_block):
        d_out = torch.zeros((N_UNITS * N_OUT, N_FREQ, N_BEAMS), dtype=torch.float32, device="cuda")
        bf.set_weights_device(d_weights)
        bf.beamform(d_block, N_UNITS, d_out)
        torch.cuda.synchronize()
        return d_out.cpu().numpy().astype(np.float64).sum(axis=0)             # [f][b]

    scale = float(np.float32(1.0 / 127.0)) ** 2
    p_null, p_orig = power(d_w, d_rfi), power(d_w_in, d_rfi)
    for got, weights in ((p_null, orc["w_null"]), (p_orig, orc["w"])):       # (a) for the beamformer: exact integers
        want = exact_power(sc["rfi_only"], weights) * scale
        assert np.all(np.abs(got - want) <= 2 * n_ipo * 2.0 ** -24 * want + 1e-30)
    ratio = p_null[0].sum() / p_orig[0].sum()
    print("interferer power, nulled / original, summed over %d beams: %.5f (k_f = %.4f)" % (N_BEAMS, ratio, orc["k"][0]))
    assert p_orig[0].sum() > 0 and ratio <= 1.0 / 20                         # (b)
    # (d)
    s_null, s_orig = power(d_w, d_src)[0, 0], power(d_w_in, d_src)[0, 0]
    v = corr_oracle.RE[orc["src"][:, 0]] + 1j * corr_oracle.IM[orc["src"][:, 0]]          # [unit][time][ant]
    wf = orc["k"][0] * (orc["w_f"][0, :, 0, 0] + 1j * orc["w_f"][0, :, 0, 1])
    y = np.abs(v @ wf)
    e_t = np.sqrt(0.5) * np.abs(v).sum(axis=-1)
    p_f, bound = (y * y).sum() * scale, (2 * y * e_t + e_t * e_t).sum() * scale
    print("test source, beam 0: device %.6g, unquantised k_f w' %.6g (bound %.3g), k_f^2 x original %.6g" % (s_null, p_f, bound, orc["k"][0] ** 2 * s_orig))
    assert abs(s_null - p_f) <= bound + 2 * n_ipo * 2.0 ** -24 * s_null
    assert np.linalg.norm(orc["s"]) > 4 and abs(s_null / (orc["k"][0] ** 2 * s_orig) - 1) <= 0.05
    bf.close()


def test_beam_solve_mode_and_apply(torch, bfmod, tmp_path):
    """`beam -j 27 -a 1 -V vis.bin` as tests/test_gpu_corr.py runs it, then `beam -E vis.bin -Z null.bin -y 2`: both records equal the
    oracle on host.read_vis_file's records to the bit in every 16th channel and the last (the junk source is noise, so every vector takes
    all 200 multiplications: the oracle needs a second per 16 channels) and are finite with n_used = 0 everywhere.  The DEBUG run with -Z,
    and with -A ... -Z, completes, and the library's DEBUG flow with the same files (the flow `beam` calls) writes the same table and
    reports the weights it set: the oracles applied in that order, calibration first.  Observation mode: a null file with nothing to
    null (n_used = 0 in every channel) leaves the -w stream byte-identical to the run without -Z.  Two loopback ranks write vis.bin.0 / .1
    and `beam -E vis.bin -Z null.bin -R 2 -r k` turns them into null.bin.0 / .1 with their own FIRST_CHANNEL."""
    import subprocess

    from dsabeamformer_amd import build, host

    vis_path, null_path = str(tmp_path / "vis.bin"), str(tmp_path / "null.bin")
    r = subprocess.run([build.BEAM, "-j", "27", "-a", "1", "-V", vis_path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    vhdr, dumps = host.read_vis_file(vis_path)
    assert len(dumps) == 2
    n_ant, n_freq = int(vhdr["NANT"]), int(vhdr["NFREQ"])
    r = subprocess.run([build.BEAM, "-E", vis_path, "-Z", null_path, "-y", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Wrote 2 null records" in r.stdout, r.stdout + r.stderr
    nhdr, recs = host.read_null_file(null_path)
    assert nhdr["CONTENT"] == "nullvecs" and nhdr["DTYPE"] == "float64" and nhdr["LAYOUT"] == "freq,vec,ant,reim"
    assert (int(nhdr["NANT"]), int(nhdr["NFREQ"]), int(nhdr["FIRST_CHANNEL"]), int(nhdr["NNULL"])) == (n_ant, n_freq, 0, 2)
    assert len(recs) == 2
    some = sorted(set(range(0, n_freq, 16)) | {n_freq - 1})
    for (first_block, n_columns, vis), (b, c, vecs, eig, info) in zip(dumps, recs):
        want = null_oracle.solve(np.ascontiguousarray(vis[some]), n_ant, n_null=2)
        assert (b, c) == (first_block, n_columns)
        _same((_bits(vecs[some]), _bits(eig[some]), info[some]), want, "beam -E -Z")
        assert np.isfinite(vecs).all() and np.isfinite(eig).all() and not info[:, 0].any() and not vecs.any()
    # ---- -Z in the DEBUG run: a null file of the DEBUG geometry, two orthonormal vectors per channel, 0, 1 or 2 of them used
    dbg = bfmod.debug_config()
    rng = np.random.default_rng(31)
    z = rng.standard_normal((dbg.n_freq, dbg.n_ant, 2)) + 1j * rng.standard_normal((dbg.n_freq, dbg.n_ant, 2))
    q = np.linalg.qr(z)[0].transpose(0, 2, 1)                                # [freq][2][ant]
    vecs = np.stack([q.real, q.imag], axis=-1)
    info = np.zeros((dbg.n_freq, 5), np.int32)
    info[:, 0] = np.arange(dbg.n_freq) % 3
    vecs[info[:, 0] < 2, 1] = 0.0
    vecs[info[:, 0] < 1, 0] = 0.0
    apply_null = str(tmp_path / "apply_null.bin")
    eig = np.zeros((dbg.n_freq, 3))
    host.write_null_file(apply_null, n_ant=dbg.n_ant, n_freq=dbg.n_freq, first_channel=0, n_null=2,
                         records=[(0, 1, np.zeros_like(vecs), eig, np.zeros_like(info)), (1, 1, vecs, eig, info)])   # the LAST record counts
    amp = rng.uniform(0.5, 1.5, size=(1, dbg.n_freq, dbg.n_ant))
    g = amp * np.exp(2j * np.pi * rng.uniform(size=amp.shape))
    layer = np.stack([g.real, g.imag], axis=-1)
    apply_gains = str(tmp_path / "apply_gains.bin")
    host.write_gains_file(apply_gains, n_ant=dbg.n_ant, n_pol=1, n_freq=dbg.n_freq, first_channel=0,
                          records=[(0, 1, layer, np.ones((1, dbg.n_freq, 2), np.int32))])
    cfgdir = os.path.join(ROOT, "tests", "golden", "config")
    files = ["-p", os.path.join(cfgdir, "linear_positions.txt"), "-d", os.path.join(cfgdir, "linear_directions.txt"),
             "-s", os.path.join(cfgdir, "linear_source_directions_1024.txt")]
    steering = host.make_weights(host.read_positions(files[1], dbg.n_ant), host.read_directions(files[3], dbg.n_beams), dbg.n_freq)
    for tag, extra, kw, start in (("null", ["-Z", apply_null], dict(nulls=apply_null), steering),
                                  ("gains+null", ["-A", apply_gains, "-Z", apply_null], dict(gains=apply_gains, nulls=apply_null),
                                   cal_oracle.calibrate_weights(steering, layer[0]))):
        out_cli, out_lib = str(tmp_path / (tag + "_cli.py")), str(tmp_path / (tag + "_lib.py"))
        r = subprocess.run([build.BEAM] + files + extra + ["-o", out_cli], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "interferer vectors per channel out of the weights" in r.stdout and os.path.getsize(out_cli) > 0, r.stdout + r.stderr
        assert ("Calibrated the weights" in r.stdout) == ("-A" in extra)
        res = host.run_debug_observation(dbg, positions=files[1], directions=files[3], sources=files[5], output=out_lib, return_weights=True, **kw)
        assert open(out_lib).read() == open(out_cli).read()
        want_w, _ = null_oracle.project(start, vecs, info)
        assert np.array_equal(res["weights"], want_w), tag
        assert np.array_equal(res["weights"][0::3], start[0::3]) and not np.array_equal(res["weights"][1::3], start[1::3])
    # ---- observation mode: nothing to null, nothing changes
    pcfg = bfmod.production_config()
    idle = str(tmp_path / "idle.bin")
    host.write_null_file(idle, n_ant=pcfg.n_ant, n_freq=pcfg.n_freq, first_channel=0, n_null=1,
                         records=[(0, 1, np.zeros((pcfg.n_freq, 1, pcfg.n_ant, 2)), np.zeros((pcfg.n_freq, 2)), np.zeros((pcfg.n_freq, 3), np.int32))])
    streams = []
    for tag, extra in (("plain", []), ("idle", ["-Z", idle])):
        det = str(tmp_path / (tag + ".det"))
        r = subprocess.run([build.BEAM, "-j", "26", "-w", det] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and ("out of the weights" in r.stdout) == bool(extra), r.stdout + r.stderr
        streams.append(open(det, "rb").read())
        os.remove(det)
    assert len(streams[0]) > 4096 and streams[0] == streams[1]
    # ---- two loopback ranks
    from test_gpu_multirank import FAKE  # noqa: F401  (built by that module's fixture; build here if it has not run)

    src = os.path.join(SUPPORT, "fake_rccl.cpp")
    if not os.path.exists(FAKE) or os.path.getmtime(FAKE) < os.path.getmtime(src):
        obj = os.path.join(SUPPORT, "fake_rccl.o")
        subprocess.check_call([build.HIPCC, "-O2", "-std=c++17", "-fPIC", "-c", src, "-o", obj])
        cxx = os.path.join(os.path.dirname(os.path.realpath(build.HIPCC)), "..", "lib", "llvm", "bin", "clang++")
        subprocess.check_call([cxx if os.path.exists(cxx) else "g++", "-shared", "-fPIC", "-o", FAKE, obj, "-lpthread", "-lrt"])
    svis, snull = str(tmp_path / "svis.bin"), str(tmp_path / "snull.bin")
    cmd = lambda rk: [build.BEAM, "-j", "26", "-D", "0", "-R", "2", "-r", str(rk), "-I", str(tmp_path / "id"), "-V", svis]  # noqa: E731
    procs = [subprocess.Popen(cmd(rk), env=dict(os.environ, DSABF_RCCL_LIB=FAKE), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for rk in (0, 1)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    for rk in (0, 1):
        r = subprocess.run([build.BEAM, "-E", svis, "-Z", snull, "-R", "2", "-r", str(rk), "-y", "1:0"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "Wrote 1 null records to %s.%d" % (snull, rk) in r.stdout, r.stdout + r.stderr
        shdr, srecs = host.read_null_file("%s.%d" % (snull, rk))
        _, sdumps = host.read_vis_file("%s.%d" % (svis, rk))
        assert (int(shdr["NFREQ"]), int(shdr["FIRST_CHANNEL"]), int(shdr["NNULL"])) == (pcfg.n_freq // 2, rk * pcfg.n_freq // 2, 1)
        few = [0, pcfg.n_freq // 2 - 1]
        want = null_oracle.solve(np.ascontiguousarray(sdumps[0][2][few]), pcfg.n_ant, min_ratio=0.0)
        _same((_bits(srecs[0][2][few]), _bits(srecs[0][3][few]), srecs[0][4][few]), want, "rank %d" % rk)
        assert np.all(srecs[0][4][:, 0] == 1)                                # min_ratio 0: every channel's vector is used
    assert not os.path.exists(snull)
