"""GPU tests (-m gpu) of the full-Stokes follow-up beams (include/dsabf.h: bf_stokes_*; docs/STOKES.md).  The reference is
tests/support/stokes_oracle.py -- a nibble table, an int64 einsum and a reshape-sum -- and every comparison of Stokes parameters is
np.array_equal on whole sentinel-filled outputs: the sums are exact integers, so there is no tolerance to state.  The one comparison
with a tolerance is Stokes I against the float32 detected stream, at the bound include/dsabf.h states for the canonical detect.

Every test is ONE function that loops over its cases, as tests/test_gpu_sk.py does: the sweep cap of conftest.py thins parametrised
cases, and none of these may be left out."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

SUPPORT = os.path.join(ROOT, "tests", "support")
sys.path.insert(0, SUPPORT)
import stokes_oracle as so  # noqa: E402

pytestmark = pytest.mark.gpu

BF_ERR_INVALID, BF_ERR_STATE = -1, -4
SENTINEL = -0x0123456789ABCDEF


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need a GPU"
    return t


@pytest.fixture(scope="module")
def bfmod():
    import dsabeamformer_amd as m

    return m


def _cfg(bfmod, n_ant, n_avg, n_out, n_beams=32, n_freq=3, **over):
    kw = dict(n_ant=n_ant, n_pol=2, n_avg=n_avg, n_beams=n_beams, n_freq=n_freq, n_out_per_gemm=n_out, n_gemms_per_block=4,
              n_blocks_on_gpu=2, n_streams=4)
    kw.update(over)
    return bfmod.debug_config(**kw)


def _random_packed(rng, cfg, n_units):
    return rng.integers(0, 256, size=(n_units, cfg.n_freq, cfg.n_out_per_gemm * 2 * cfg.n_avg, cfg.n_ant), dtype=np.uint8)


def _random_weights(rng, cfg):
    return rng.integers(-128, 128, size=(cfg.n_freq, cfg.n_ant, cfg.n_beams, 2), dtype=np.int8)


def _run(torch, stage, packed, n_units, want_shape):
    """bf_stokes_device into a sentinel-filled output with a guard cell behind it; returns the output and checks the guard."""
    n = int(np.prod(want_shape))
    d_out = torch.full((n + 4,), SENTINEL, dtype=torch.int64, device="cuda")
    stage.compute(torch.from_numpy(packed).cuda(), n_units, d_out)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[n:] == SENTINEL).all()
    return got[:n].reshape(want_shape)


def _compare(got, want, case):
    assert got.shape == want.shape, (case, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (case, len(bad), bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])


# (n_ant, beams, n_avg, n_out, n_int, n_freq, n_units); n_beams is 32.  "S" as n_int: the whole unit in one window.
# 16-byte loads where n_ant % 16 == 0 (16, 64, 256), 4-byte loads otherwise; 68, 100, 132: a partial last 64-antenna step; 132 and 256:
# three and four steps.  S = n_out * n_avg: 1 and 3 (a partial 16-column tile), 8, 16, 24, 48, 128.  n_int 3 with S = 24, 48: windows that
# straddle tiles and lanes.  Spans of fewer than 8 windows at the end of a unit: (S / n_int) % 8 != 0 in several cases.
DESC16 = list(range(31, 15, -1))
SHAPE_CASES = [(4, [0], 1, 1, 1, 1, 1), (4, [31, 0, 7], 1, 3, 1, 3, 3), (4, [5], 1, 3, 3, 1, 1), (4, DESC16, 16, 8, 16, 3, 1),
               (16, [31, 30, 2], 1, 8, 1, 3, 3), (16, [0], 16, 1, 2, 1, 3), (20, DESC16, 1, 8, 8, 3, 1), (20, [9, 3, 31], 8, 3, 3, 1, 3),
               (64, DESC16, 16, 8, 16, 3, 3), (64, [31], 16, 8, 1, 1, 1), (64, [0, 31, 1], 16, 3, 3, 3, 1), (64, [2, 1, 0], 1, 8, 2, 1, 3),
               (68, [31, 0, 15], 16, 1, 8, 3, 1), (68, DESC16, 8, 3, 24, 1, 3), (100, [1], 16, 3, 2, 3, 3), (100, [30, 31, 0], 1, 1, 1, 1, 1),
               (132, DESC16, 16, 1, 16, 1, 3), (132, [4, 2, 9], 8, 3, 3, 3, 1), (256, [31], 16, 8, "S", 3, 1), (256, DESC16, 1, 3, 1, 1, 3),
               (256, [0, 16, 31], 16, 3, 8, 3, 3),
               # every (k-steps, 16-byte loads) pair of stokes_kernel with n_int 1 (direct) and with a cooperative n_int: 80 ... 128 and 144 ... 192
               # antennas with n_ant % 16 == 0 are two and three steps on 16-byte loads, 196 ... 252 four steps on 4-byte loads; 128 antennas on
               # BASELINE's windows (n_avg 16 and 1); 132 with n_int 1 (three steps, 4-byte loads, direct)
               (128, DESC16, 16, 8, 16, 3, 1), (128, [31, 0, 7], 1, 8, 1, 3, 3), (80, [0, 31, 1], 1, 3, 1, 1, 1), (112, [5], 8, 3, 3, 1, 3),
               (144, DESC16, 1, 8, 1, 1, 3), (144, [9], 16, 3, 8, 3, 1), (192, [31, 0, 15], 16, 1, 2, 3, 3), (192, DESC16, 1, 3, 1, 3, 1),
               (196, [2], 8, 3, 24, 1, 3), (196, [0, 16, 31], 1, 8, 1, 3, 1), (252, DESC16, 16, 8, "S", 1, 1), (252, [31], 1, 1, 1, 3, 3),
               (132, [7, 0, 31], 1, 8, 1, 3, 1)]
# More spans than one round of workgroups holds (8 workgroups per CU on 256 CUs, 4 waves each: 8192): n_int = 1 at 64 antennas has 16 spans
# per unit and channel (3 * 172 * 16 = 8256); n_int = 16 at 4 antennas one (3 * 2800 = 8400).  Ranges are cut by the cap and cross channels.
# Launches with fewer spans than 8 waves per CU (2048 on 256 CUs) and n_int > 1 are cooperative -- a span per workgroup: every case of
# SHAPE_CASES with n_int > 1.  Every case behind the first has 2100 spans or more and n_int > 1 -- 16, 3, 2 and S: a span per wave.  The last
# four: two, three and four steps on 16-byte loads and four steps on 4-byte loads (128, 192, 256 and 252 antennas), one span per unit and channel.
LARGE_CASES = [(64, [31, 0, 7], 16, 8, 1, 3, 172), (4, [3, 31], 16, 8, 16, 3, 2800),
               (64, [0, 31, 5], 16, 8, 16, 3, 700), (20, [9, 3, 31], 8, 3, 3, 3, 700), (68, [2, 1, 0], 1, 8, 2, 1, 2100), (132, [31], 16, 1, "S", 3, 700),
               (128, [0, 31, 5], 1, 8, 2, 3, 700), (192, [9, 3, 31], 1, 3, 3, 3, 700), (252, [2], 1, 8, 8, 1, 2100), (256, [31, 16, 0], 16, 1, 16, 3, 700)]


def test_every_shape_to_the_bit(torch, bfmod):
    """bf_stokes_device against the oracle on random bytes (every code) and random weights over all of int8."""
    from dsabeamformer_amd import api

    for lst, idx in (((4, 16, 20, 64, 68, 80, 100, 112, 128, 132, 144, 192, 196, 252, 256), 0), ((1, 8, 16), 2), ((1, 3, 8), 3), ((1, 3), 5), ((1, 3), 6)):
        assert {c[idx] for c in SHAPE_CASES} == set(lst), idx
    assert {len(c[1]) for c in SHAPE_CASES} == {1, 3, 16} and {c[4] for c in SHAPE_CASES} >= {1, 2, 3, 8, 16, "S"}
    assert any(0 in c[1] for c in SHAPE_CASES) and any(31 in c[1] for c in SHAPE_CASES)
    for group in ((80, 112, 128), (144, 192), (196, 252)):   # direct and cooperative, 1 / 3 / 16 beams at every new class of antenna counts
        mine = [c for c in SHAPE_CASES if c[0] in group]
        assert {len(c[1]) for c in mine} == {1, 3, 16} and any(c[4] == 1 for c in mine) and any(c[4] != 1 for c in mine), group
    assert {(c[0], c[2]) for c in SHAPE_CASES} >= {(128, 16), (128, 1)} and {c[0] for c in LARGE_CASES[-4:]} == {128, 192, 252, 256}
    rng = np.random.default_rng(20261019)
    t0, n = time.perf_counter(), 0
    for case in SHAPE_CASES + LARGE_CASES:
        n_ant, beams, n_avg, n_out, n_int, n_freq, n_units = case
        cfg = _cfg(bfmod, n_ant, n_avg, n_out, n_freq=n_freq)
        S = n_out * n_avg
        n_int = S if n_int == "S" else n_int
        packed, w = _random_packed(rng, cfg, n_units), _random_weights(rng, cfg)
        want = so.stokes(packed, w, beams, n_int, so.geometry(cfg))
        bf = bfmod.Beamformer(cfg)
        stage = api.StokesBeams(bf, n_int)
        stage.set_weights(w, beams)
        assert stage.entries * n_units * 4 == want.size, case
        api.stage_launches(clear=True)
        _compare(_run(torch, stage, packed, n_units, want.shape), want, case)
        # which stokes_kernel<k-steps, 16-byte loads, mode> the launcher took: mode 0 direct, 1 a span per wave, 2 cooperative
        name = "stokes_kernel<%d, %s, %d>" % ((n_ant + 63) // 64, "true" if n_ant % 16 == 0 else "false",
                                              0 if n_int == 1 else 1 if case in LARGE_CASES else 2)
        assert [k for k in api.stage_launches() if k.startswith("stokes_kernel<")] == [name], (case, api.stage_launches())
        stage.close()
        bf.close()
        n += want.size
    print("stokes_kernel: %d cases, %d int64 compared, %.1f s" % (len(SHAPE_CASES) + len(LARGE_CASES), n, time.perf_counter() - t0))


def test_every_byte_code_and_weight_extreme(torch, bfmod):
    """Antenna a sees code (c + a) % 256 at column c, so every code meets every byte position of a lane's word; the weights are drawn
    from the extremes of int8 in both parts.  64 antennas (one whole step) and 68 (a partial one, 4-byte loads)."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(23)
    for n_ant in (64, 68):
        cfg = _cfg(bfmod, n_ant, 16, 8, n_freq=2)                                # 256 columns per unit and channel
        c, a = np.meshgrid(np.arange(256), np.arange(n_ant), indexing="ij")
        packed = np.broadcast_to(((c + a) % 256).astype(np.uint8), (2, 2, 256, n_ant)).copy()
        w = rng.choice(np.array([-128, -127, -1, 0, 1, 127], np.int8), size=(2, n_ant, 32, 2))
        beams = [31, 0, 16, 5]
        bf = bfmod.Beamformer(cfg)
        for n_int in (1, 16):
            want = so.stokes(packed, w, beams, n_int, so.geometry(cfg))
            stage = api.StokesBeams(bf, n_int)
            stage.set_weights(torch.from_numpy(w).cuda(), beams)                 # (the gather kernel)
            _compare(_run(torch, stage, packed, 2, want.shape), want, (n_ant, n_int))
            stage.close()
        bf.close()


def test_the_int32_bound(torch, bfmod):
    """256 antennas, every voltage 0x88 = (-8, -8).  Weights all (-128, -128): X = Y = (0, 2^19), the largest imaginary part; weights all
    (-128, 127): re = 256 (1024 + 1016) = 522240, the largest real part.  Expected values in Python integers, one window per unit."""
    from dsabeamformer_amd import api

    cfg = _cfg(bfmod, 256, 16, 8, n_freq=1)
    S = 128
    packed = np.full((1, 1, 2 * S, 256), 0x88, np.uint8)
    bf = bfmod.Beamformer(cfg)
    stage = api.StokesBeams(bf, S)
    for (wr, wi) in ((-128, -128), (-128, 127)):
        w = np.empty((1, 256, 32, 2), np.int8)
        w[..., 0], w[..., 1] = wr, wi
        re, im = 256 * (-8 * wr - -8 * wi), 256 * (-8 * wr + -8 * wi)
        assert (re, im) == ((0, 2 ** 19) if wi == -128 else (522240, 2048))
        power = re * re + im * im
        want = np.empty((1, 1, 1, 2, 4), np.int64)
        want[...] = (2 * S * power, 0, 2 * S * power, 0)                         # Y = X: Q = V = 0, U = I
        stage.set_weights(w, [0, 31])
        _compare(_run(torch, stage, packed, 1, want.shape), want, (wr, wi))
        assert int(want[0, 0, 0, 0, 0]) == 2 * S * power > 2 ** 45               # (far past int32)
    stage.close()
    bf.close()


def test_polarisation_identities_on_the_device(torch, bfmod):
    """Y = X gives Q = V = 0 and U = I; Y = i X gives Q = U = 0 and V = -I (the oracle's scenes, voltages -7 ... 7)."""
    from dsabeamformer_amd import api

    cfg = _cfg(bfmod, 100, 2, 8)
    bf = bfmod.Beamformer(cfg)
    for n_int in (1, 4):
        stage = api.StokesBeams(bf, n_int)
        for relation in ("equal", "quarter"):
            packed, w = so.scene(31, so.geometry(cfg), 2, relation)
            stage.set_weights(w, [7, 31, 0])
            got = _run(torch, stage, packed, 2, (2, 16 // n_int, 3, 3, 4))
            _compare(got, so.stokes(packed, w, [7, 31, 0], n_int, so.geometry(cfg)), (n_int, relation))
            assert got[..., 0].min() > 0 and not got[..., 1].any()
            if relation == "equal":
                assert not got[..., 3].any() and np.array_equal(got[..., 2], got[..., 0])
            else:
                assert not got[..., 2].any() and np.array_equal(got[..., 3], -got[..., 0])
        stage.close()
    bf.close()


def test_stokes_I_is_the_detected_stream(torch, bfmod):
    """n_int = n_avg: alpha^2 I against column beam_k of bf_beamform_device, within (n_ipo + 4) 2^-24 relative -- the bound
    include/dsabf.h states for the canonical detect (derived there, not measured here)."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(29)
    a2 = np.float64(np.float32(1.0 / 127)) ** 2
    for n_ant in (64, 132):
        cfg = _cfg(bfmod, n_ant, 16, 8, n_beams=32, n_freq=3)
        packed, w = _random_packed(rng, cfg, 2), rng.integers(-127, 128, size=(3, n_ant, 32, 2), dtype=np.int8)
        beams = [31, 0, 9, 16]
        bf = bfmod.Beamformer(cfg)
        bf.set_weights(w)
        stage = api.StokesBeams(bf)                                              # n_int None: n_avg
        assert stage.n_int == 16
        stage.set_weights(w, beams)
        d_in = torch.from_numpy(packed).cuda()
        d_det = torch.zeros((2, 8, 3, 32), dtype=torch.float32, device="cuda")
        bf.beamform(d_in, 2, d_det)
        got = _run(torch, stage, packed, 2, (2, 8, 3, 4, 4))
        det = d_det.cpu().numpy().astype(np.float64)[..., beams]
        want = a2 * got[..., 0].astype(np.float64)
        tol = (2 * 16 + 4) * 2.0 ** -24
        rel = np.abs(det - want) / want
        print("n_ant %d: largest relative difference %.3g, bound %.3g" % (n_ant, rel.max(), tol))
        assert want.min() > 0 and rel.max() <= tol, (n_ant, rel.max(), tol)
        stage.close()
        bf.close()


def test_refusals_launch_nothing(torch, bfmod):
    """Every BF_ERR_INVALID / BF_ERR_STATE case of the contract; the output keeps its sentinels and nothing becomes pending."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(37)
    cfg = _cfg(bfmod, 64, 2, 4)                                                  # S = 8, 4 units per block
    packed, w = _random_packed(rng, cfg, 5), _random_weights(rng, cfg)
    d_in, d_w = torch.from_numpy(packed).cuda(), torch.from_numpy(w).cuda()
    d_out = torch.full((5 * 8 * 3 * 16 * 4,), SENTINEL, dtype=torch.int64, device="cuda")

    def refused(code, call, msg=None):
        with pytest.raises(bfmod.DsabfError) as e:
            call()
        assert e.value.code == code, (e.value.code, str(e.value))
        assert msg is None or str(e.value) == "libdsabf error %d: %s" % (code, msg), str(e.value)

    mono = bfmod.Beamformer(_cfg(bfmod, 64, 2, 4, n_pol=1))                      # n_pol != 2
    refused(BF_ERR_INVALID, lambda: api.StokesBeams(mono, 1))
    mono.close()
    wide = bfmod.Beamformer(_cfg(bfmod, 260, 2, 4))                              # n_ant > 256
    refused(BF_ERR_INVALID, lambda: api.StokesBeams(wide, 1))
    wide.close()
    bf = bfmod.Beamformer(cfg)
    for n_int in (0, -1, 3, 16):                                                 # n_int that does not divide S = 8
        refused(BF_ERR_INVALID, lambda: api.StokesBeams(bf, n_int))
    refused(BF_ERR_INVALID, lambda: api.StokesBeams(bf, 1, max_in_flight=0))
    stage = api.StokesBeams(bf, 2, max_in_flight=2)
    refused(BF_ERR_STATE, lambda: stage.compute(d_in, 1, d_out))                 # before any weights
    refused(BF_ERR_STATE, lambda: stage.push(d_in, 1))
    for beams in ([], list(range(17)), [0, 32], [-1], [31, 5, 32]):              # K outside 1 ... 16, an index outside [0, n_beams)
        refused(BF_ERR_INVALID, lambda: stage.set_weights(w, beams))
        refused(BF_ERR_INVALID, lambda: stage.set_weights(d_w, beams))
    refused(BF_ERR_STATE, lambda: stage.push(d_in, 1))                           # (a refused selection sets nothing)
    stage.set_weights(w, [3, 1])
    refused(BF_ERR_INVALID, lambda: stage.push(d_in, 5))                         # more than n_gemms_per_block units
    refused(BF_ERR_INVALID, lambda: stage.push(d_in, 0))
    refused(BF_ERR_INVALID, lambda: stage.compute(d_in, 0, d_out))
    refused(BF_ERR_INVALID, lambda: stage.compute(d_in.data_ptr() + 4, 1, d_out))
    refused(BF_ERR_INVALID, lambda: stage.compute(d_in, 1, d_out.data_ptr() + 8))
    refused(BF_ERR_STATE, stage.collect, "bf_stokes_collect: no push is pending")
    assert stage.pending == 0
    stage.push(d_in, 1)
    stage.push(d_in, 1)
    refused(BF_ERR_STATE, lambda: stage.push(d_in, 1),                           # max_in_flight uncollected sets
            "bf_stokes_push: 2 result sets are uncollected (max_in_flight): bf_stokes_collect first")
    refused(BF_ERR_STATE, lambda: stage.set_weights(w, [3, 1, 2]),               # more beams than before: the sets would grow under the pending ones
            "bf_stokes_set_weights: 3 beams are more than any selection before (2), so the result sets grow: collect the 2 pending ones first")
    assert stage.pending == 2
    want = so.stokes(packed[:1], w, [3, 1], 2, so.geometry(cfg))
    for _ in range(2):
        _compare(stage.collect(), want, "after the refusals")
    torch.cuda.synchronize()
    assert bool((d_out == SENTINEL).all())
    stage.close()
    bf.close()


def test_new_weights_apply_to_later_pushes(torch, bfmod):
    """push, set_weights_device with other beams on ANOTHER stream, push -- no host synchronisation in between: the first set holds the
    old beams, the second the new ones (the gather waits on the device for the first kernel, the second kernel for the gather)."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(43)
    cfg = _cfg(bfmod, 256, 16, 8, n_freq=8)                                      # 4 units of 2 MiB: a kernel long enough to still be running
    packed, w = _random_packed(rng, cfg, 4), _random_weights(rng, cfg)
    w2 = _random_weights(rng, cfg)
    d_in, d_w2 = torch.from_numpy(packed).cuda(), torch.from_numpy(w2).cuda()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    bf = bfmod.Beamformer(cfg)
    stage = api.StokesBeams(bf, 1, max_in_flight=3)
    old, new, third = [1, 2, 3], [30, 2, 9], [4, 5]
    stage.set_weights(w, old)
    torch.cuda.synchronize()
    stage.push(d_in, 4, s1.cuda_stream)
    stage.set_weights(d_w2, new, s2.cuda_stream)
    stage.push(d_in, 4, s1.cuda_stream)
    stage.set_weights(d_w2, third, s1.cuda_stream)                               # fewer beams: no growth, nothing to drain
    stage.push(d_in, 4, s2.cuda_stream)
    g = so.geometry(cfg)
    _compare(stage.collect(), so.stokes(packed, w, old, 1, g), "old")
    _compare(stage.collect(), so.stokes(packed, w2, new, 1, g), "new")
    _compare(stage.collect(), so.stokes(packed, w2, third, 1, g), "third")
    stage.close()
    bf.close()


def test_weight_writes_are_ordered_across_queues(torch, bfmod):
    """The ONE copy of the weights is written in call order and never under a reader, whichever queues are used.  Stream s1 is kept busy
    with matrix products (tens of milliseconds), so that what is queued on it runs long after the host calls that follow:
    (1) set_weights_device(A) on busy s1, then set_weights_device(B) on idle s2, then the host form (C) -- each later write waits for
        the one before it, so a push after each sees ITS weights and gather A cannot land on top of B;
    (2) bf_stokes_device on busy s1 with weights C, then set_weights_device(A) on idle s2: the gather waits for that kernel too."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(47)
    cfg = _cfg(bfmod, 64, 16, 8, n_freq=4)
    g = so.geometry(cfg)
    packed = _random_packed(rng, cfg, 2)
    wa, wb, wc = (_random_weights(rng, cfg) for _ in range(3))
    ba, bb, bc = [1, 2, 3], [30, 2, 9], [7, 31, 0]
    d_in, d_wa, d_wb = torch.from_numpy(packed).cuda(), torch.from_numpy(wa).cuda(), torch.from_numpy(wb).cuda()
    big = torch.randn((8192, 8192), device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    bf = bfmod.Beamformer(cfg)
    stage = api.StokesBeams(bf, 16, max_in_flight=3)
    stage.set_weights(wc, bc)
    n = 2 * stage.entries * 4
    d_direct = torch.full((n,), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def keep_busy():
        with torch.cuda.stream(s1):
            for _ in range(4):
                torch.mm(big, big)

    keep_busy()
    stage.set_weights(d_wa, ba, s1.cuda_stream)                                  # runs when s1 gets to it
    stage.set_weights(d_wb, bb, s2.cuda_stream)                                  # must wait for gather A
    stage.push(d_in, 2, s2.cuda_stream)
    stage.set_weights(wc, bc)                                                    # the host form: behind gather B and that push
    stage.push(d_in, 2, s2.cuda_stream)
    keep_busy()
    stage.compute(d_in, 2, d_direct, s1.cuda_stream)                             # reads C, long after this call returns
    stage.set_weights(d_wa, ba, s2.cuda_stream)                                  # must wait for that kernel
    stage.push(d_in, 2, s2.cuda_stream)
    _compare(stage.collect(), so.stokes(packed, wb, bb, 16, g), "B after A on a busy queue")
    _compare(stage.collect(), so.stokes(packed, wc, bc, 16, g), "the host form after B")
    _compare(stage.collect(), so.stokes(packed, wa, ba, 16, g), "A after a direct kernel")
    torch.cuda.synchronize()
    _compare(d_direct.cpu().numpy().reshape(2, 8, 4, 3, 4), so.stokes(packed, wc, bc, 16, g), "the direct kernel under a later gather")
    stage.close()
    bf.close()


def test_pushes_on_two_queues_and_the_in_flight_limit(torch, bfmod):
    """Ragged pushes alternately on two streams with no host synchronisation, max_in_flight 2: the push beyond it is refused and queues
    nothing, the sets come back in order, each the oracle over its own units; then the handle is destroyed first."""
    from dsabeamformer_amd import api

    rng = np.random.default_rng(17)
    cfg = _cfg(bfmod, 68, 8, 3, n_freq=5)                                        # S = 24, windows of 3
    packed, w = _random_packed(rng, cfg, 16), _random_weights(rng, cfg)
    per_unit = packed[0].size
    beams = [31, 4, 0]
    want = so.stokes(packed, w, beams, 3, so.geometry(cfg))
    bf = bfmod.Beamformer(cfg)
    stage = api.StokesBeams(bf, 3, max_in_flight=2)
    stage.set_weights(w, beams)
    d_in = torch.from_numpy(packed).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    at, queued, refused = 0, [], 0
    for k, c in enumerate([1, 4, 2, 3, 1, 4, 1]):
        if stage.pending == 2:
            with pytest.raises(bfmod.DsabfError) as e:
                stage.push(d_in.data_ptr() + at * per_unit, c, streams[k % 2].cuda_stream)
            assert e.value.code == BF_ERR_STATE and stage.pending == 2
            assert str(e.value) == "libdsabf error -4: bf_stokes_push: 2 result sets are uncollected (max_in_flight): bf_stokes_collect first"
            refused += 1
            lo, hi = queued.pop(0)
            _compare(stage.collect(), want[lo:hi], (lo, hi))
        stage.push(d_in.data_ptr() + at * per_unit, c, streams[k % 2].cuda_stream)
        queued.append((at, at + c))
        at += c
    assert at == 16 and refused == 5 and stage.pending == 2
    for lo, hi in queued:
        _compare(stage.collect(), want[lo:hi], (lo, hi))
    assert stage.pending == 0
    bf.close()                                                                   # the handle first: the stage answers BF_ERR_STATE and can be destroyed
    for call in (lambda: stage.push(d_in, 1), stage.collect, lambda: stage.set_weights(w, beams), lambda: stage.compute(d_in, 1, d_in)):
        with pytest.raises(bfmod.DsabfError) as e:
            call()
        assert e.value.code == BF_ERR_STATE
    stage.close()


# ---- the resident block and the driver ----------------------------------------------------------------------------------------------
N_ANALYSED = 2      # `-j 27`: the junk source counts the 25 burn-in reads, so 2 blocks are analysed
RUN_BEAMS = [0, 100, 255]
_RUN = {}           # n_freq of the geometry -> (the analysed blocks' bytes, the driver's weights): regenerated once, shared by two tests


def _the_run(host, cfg, first_channel=0):
    """The blocks a `beam -j 27` run analyses (block i is junk block (25 + i) % 4, regenerated with host.junk_bytes as tests/test_gpu_sk.py
    does) and the weights the driver sets (the default positions and directions)."""
    key = (cfg.n_freq, first_channel)
    if key not in _RUN:
        n_time = cfg.n_out_per_gemm * cfg.n_pol * cfg.n_avg
        ring = host.junk_bytes(cfg.n_ant * cfg.n_freq * n_time * cfg.n_gemms_per_block, 4, 0xD5A, cfg).reshape(
            4, cfg.n_gemms_per_block, cfg.n_freq, n_time, cfg.n_ant)
        w = host.make_weights(host.default_positions(cfg.n_ant), host.default_directions(cfg.n_beams), cfg.n_freq, first_channel, 0)
        _RUN[key] = ([ring[(25 + i) % 4] for i in range(N_ANALYSED)], w)
    return _RUN[key]


def _check_file(host, path, cfg, first_channel, n_int, blocks, w):
    hdr, records = host.read_stokes_file(path)
    assert hdr["CONTENT"] == "stokes" and hdr["DTYPE"] == "int64" and int(hdr["HDR_SIZE"]) == 4096
    assert (int(hdr["NANT"]), int(hdr["NFREQ"]), int(hdr["FIRST_CHANNEL"]), int(hdr["NINT"]), int(hdr["NSEL"])) == \
        (cfg.n_ant, cfg.n_freq, first_channel, n_int, len(RUN_BEAMS))
    assert hdr["BEAMS"] == RUN_BEAMS and hdr["LAYOUT"] == "unit,time,freq,beam,iquv"
    n_u = cfg.n_gemms_per_block
    assert sum(r[1] for r in records) == N_ANALYSED * n_u and [r[0] for r in records] == list(np.cumsum([0] + [r[1] for r in records[:-1]]))
    got = np.concatenate([r[2] for r in records])
    for i, block in enumerate(blocks):
        _compare(got[i * n_u:(i + 1) * n_u], so.stokes(block, w, RUN_BEAMS, n_int, so.geometry(cfg)), (path, i))


def test_push_block_and_the_observation_loop(torch, bfmod, tmp_path):
    """bf_submit_block, bf_enqueue_block, bf_stokes_push_block on the same queue for two blocks on alternating slots: every set equals the
    oracle over its units of the submitted bytes.  Then `beam -j 27 -a 1 -x s.bin -b 0,100,255` with -l 1 and -l 16: the records equal
    the oracle over the junk source's blocks, and the detected stream written with -w beside it is byte-identical to a run without -x."""
    from dsabeamformer_amd import api, build, host

    rng = np.random.default_rng(41)
    cfg = _cfg(bfmod, 100, 2, 8)                                                 # S = 16, 4 units per block
    n_u = cfg.n_gemms_per_block
    blocks = np.stack([_random_packed(rng, cfg, n_u) for _ in range(2)])
    w = rng.integers(-127, 128, size=(cfg.n_freq, cfg.n_ant, cfg.n_beams, 2), dtype=np.int8)
    bf = bfmod.Beamformer(cfg)
    bf.set_weights(w)
    stage = api.StokesBeams(bf, 2, max_in_flight=3)
    stage.set_weights(w, [31, 0])
    pin = torch.from_numpy(blocks).pin_memory()
    for slot in (0, 1):
        bf.submit_block(slot, pin[slot], blocks[slot].nbytes)
    bf.sync(-1)
    launches = [(0, 0, n_u), (1, 0, 1), (1, 1, n_u - 1)]                         # the second block in two launches, as units_per_launch would
    for slot, first, n in launches:
        bf.enqueue_block(slot, slot, first, n, None)
        stage.push_block(slot, slot, first, n)
    for slot, first, n in launches:
        _compare(stage.collect(), so.stokes(blocks[slot][first:first + n], w, [31, 0], 2, so.geometry(cfg)), (slot, first, n))
    for bad in ((4, 0, 0, 1), (0, 2, 0, 1), (0, 0, n_u, 1), (0, 0, 1, n_u)):
        with pytest.raises(bfmod.DsabfError) as e:
            stage.push_block(*bad)
        assert e.value.code == BF_ERR_INVALID
    stage.close()
    bf.close()
    # ---- a geometry whose units are 8 bytes: odd units of the resident block start on 8-byte addresses, and are legal
    tiny = _cfg(bfmod, 4, 1, 1, n_beams=4, n_freq=1)
    tblock = _random_packed(rng, tiny, tiny.n_gemms_per_block)
    tw = _random_weights(rng, tiny)
    bf = bfmod.Beamformer(tiny)
    stage = api.StokesBeams(bf, 1, max_in_flight=4)
    stage.set_weights(tw, [3, 0])
    tpin = torch.from_numpy(tblock).pin_memory()
    bf.submit_block(0, tpin, tblock.nbytes)
    bf.sync(-1)
    for first, n in ((1, 1), (1, 2), (3, 1), (0, 4)):
        stage.push_block(0, 0, first, n)
    for first, n in ((1, 1), (1, 2), (3, 1), (0, 4)):
        _compare(stage.collect(), so.stokes(tblock[first:first + n], tw, [3, 0], 1, so.geometry(tiny)), ("tiny", first, n))
    stage.close()
    bf.close()
    # ---- the driver
    pcfg = bfmod.production_config()
    run_blocks, run_w = _the_run(host, pcfg)
    plain = tmp_path / "plain.bin"
    r = subprocess.run([build.BEAM, "-j", str(25 + N_ANALYSED), "-a", "1", "-w", str(plain)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Stokes" not in r.stdout, r.stdout + r.stderr
    for n_int in (1, 16):
        path, det = tmp_path / ("s%d.bin" % n_int), tmp_path / ("d%d.bin" % n_int)
        r = subprocess.run([build.BEAM, "-j", str(25 + N_ANALYSED), "-a", "1", "-x", str(path), "-b", "0,100,255", "-l", str(n_int), "-w", str(det)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Stokes beams: 3 beams, windows of %d samples, %d gemm-units" % (n_int, N_ANALYSED * pcfg.n_gemms_per_block) in r.stdout, r.stdout
        _check_file(host, str(path), pcfg, 0, n_int, run_blocks, run_w)
        assert open(det, "rb").read() == open(plain, "rb").read(), n_int


def test_two_loopback_ranks_write_their_own_channels(bfmod, tmp_path):
    """`beam -j 27 -R 2 -r k -x s.bin -b 0,100,255` as two shard processes (the stand-in RCCL library and launch pattern of the
    correlator's test): s.bin.0 and s.bin.1 carry FIRST_CHANNEL 0 and 128, and each equals the oracle over its rank's input with its
    rank's weights -- every shard reads the junk bytes with ITS geometry (128 channels), so both see the same bytes."""
    from test_gpu_multirank import FAKE  # noqa: F401  (built by that module's fixture; build here if it has not run)

    from dsabeamformer_amd import build, host

    src = os.path.join(SUPPORT, "fake_rccl.cpp")
    if not os.path.exists(FAKE) or os.path.getmtime(FAKE) < os.path.getmtime(src):
        obj = os.path.join(SUPPORT, "fake_rccl.o")
        subprocess.check_call([build.HIPCC, "-O2", "-std=c++17", "-fPIC", "-c", src, "-o", obj])
        cxx = os.path.join(os.path.dirname(os.path.realpath(build.HIPCC)), "..", "lib", "llvm", "bin", "clang++")
        subprocess.check_call([cxx if os.path.exists(cxx) else "g++", "-shared", "-fPIC", "-o", FAKE, obj, "-lpthread", "-lrt"])
    sfile = tmp_path / "s.bin"
    cmd = lambda rk: [build.BEAM, "-j", str(25 + N_ANALYSED), "-D", "0", "-R", "2", "-r", str(rk), "-I", str(tmp_path / "id"),  # noqa: E731
                      "-x", str(sfile), "-b", "0,100,255"]
    procs = [subprocess.Popen(cmd(rk), env=dict(os.environ, DSABF_RCCL_LIB=FAKE), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for rk in (0, 1)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert all("Stokes beams: 3 beams, windows of 16 samples" in o for o in outs), "\n".join(outs)
    assert not os.path.exists(sfile)
    shard = bfmod.production_config(n_freq=128)
    for rk in (0, 1):
        blocks, w = _the_run(host, shard, rk * 128)
        _check_file(host, str(sfile) + ".%d" % rk, shard, rk * 128, 16, blocks, w)
