"""The census of the stage kernels (csrc/<stage>/): ONE table, one row per compiled instantiation.

A row is (name, case, run): `name` is the instantiation the row claims to launch, spelled as `nm -C libdsabf.so` spells the
`__device_stub__` symbol and as the launcher records it (include/dsabf_bench.h: bf_stage_launches); `case` says in a few words what
the input is; `run(env)` builds the smallest input that selects the instantiation, runs it through the public api classes, compares
the whole output with the stage's own oracle -- to the bit, into sentinel-filled outputs with guard words behind them wherever the
caller owns the output -- and returns the number of 32-bit words it compared.  The oracles and the drivers are the ones the stages'
own tests use (tests/support/*_oracle.py, *_stage.py and the helpers of tests/test_gpu_<stage>.py); nothing is restated here.

tests/test_stage_census_cpu.py: the names of the table == tools/census.py::stage_compiled() (no GPU).
tests/test_gpu_stage_census.py: every row run, the claimed name among the names the launchers recorded during the row, and the union
of everything recorded == stage_compiled().

The edge matrices of a stage stay in its own test file; a row here is the ONE smallest launch of an instantiation."""
from __future__ import annotations

import os
import sys
from collections import namedtuple

import numpy as np

SUPPORT = os.path.dirname(os.path.abspath(__file__))
if SUPPORT not in sys.path:
    sys.path.insert(0, SUPPORT)

Row = namedtuple("Row", "name case run")
GUARD = 8            # elements of the fill value behind every output the caller owns
UINT4, UINT = "HIP_vector_type<unsigned int, 4u> ", "unsigned int"   # (the demangler's "> >")


class Env:
    """What a row needs: torch, the package, its api module, the chip's CU count, and guarded outputs."""

    def __init__(self, torch, bfmod):
        from dsabeamformer_amd import _lib, api

        self.torch, self.bfmod, self.api = torch, bfmod, api
        self.n_cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.hip = _lib._preload_hip_runtime()

    def cfg(self, **kw):
        base = dict(n_pol=2, n_avg=1, n_beams=8, n_freq=1, n_out_per_gemm=1, n_gemms_per_block=4, n_blocks_on_gpu=2, n_streams=4)
        base.update(kw)
        return self.bfmod.debug_config(**base)

    def dev(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Out:
    """A device output of `shape` filled with `fill`, GUARD more elements of the fill behind it; read() checks the guard."""

    def __init__(self, env, shape, dtype, fill):
        self.n, self.shape, self.fill = int(np.prod(shape)), tuple(shape), fill
        self.buf = env.torch.full((self.n + GUARD,), fill, dtype=getattr(env.torch, dtype), device="cuda")
        self.t = self.buf[:self.n]
        self._sync = env.torch.cuda.synchronize

    def read(self):
        self._sync()
        host = self.buf.cpu().numpy()
        assert (host[self.n:] == self.fill).all(), "a guard element behind the output was written"
        return host[:self.n].reshape(self.shape)


def same_bits(got, want, case):
    """Integer equality of the two arrays' bytes, as 32-bit words where they are whole words (a float32 as uint32, a complex64 or an
    int64 as two of them: a -0.0 or a NaN payload cannot hide); returns the number of 32-bit words compared."""
    g, w = np.ascontiguousarray(got).reshape(-1).view(np.uint8), np.ascontiguousarray(want).reshape(-1).view(np.uint8)
    assert g.size == w.size, (case, np.shape(got), np.shape(want))
    if g.size % 4 == 0:
        g, w = g.view(np.uint32), w.view(np.uint32)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (case, len(bad), bad[:4], g[bad[:4]], w[bad[:4]])
    return max(1, got.nbytes // 4)


# ---- full-Stokes beams: stokes_kernel<k-steps, 16-byte loads, mode>, stokes_gather_kernel ---------------------------------------
STOKES_ANT = {(1, True): 16, (1, False): 4, (2, True): 80, (2, False): 68, (3, True): 144, (3, False): 132, (4, True): 208, (4, False): 196}
# the launcher's modes (csrc/stokes/bf_stokes.hip): 0 direct, 1 a span per wave, 2 cooperative (a span per workgroup: fewer than 8 n_cus spans), 3 voltages
STOKES_MODES = {0: "direct: n_int 1", 1: "a span per wave: n_int 2, 8 n_cus + 52 units", 2: "cooperative: n_int 2", 3: "voltages"}
STOKES_BEAMS = [7, 0, 3]
SENTINEL64 = -0x0123456789ABCDEF
SENTINEL32 = -0x3EDCBA99


def _stokes(n_ant, mode, device_weights=False):
    def run(env):
        import stokes_oracle as so

        rng = np.random.default_rng(1000 * n_ant + mode)
        per_wave = mode == 1
        n_units = 8 * env.n_cus + 52 if per_wave else 2      # per wave: n_freq n_units spans >= 8 n_cus, one span per unit and channel
        S, n_int = (3, 1) if mode in (0, 3) else (2, 2)
        cfg = env.cfg(n_ant=n_ant, n_freq=1 if per_wave else 3, n_out_per_gemm=S)
        packed = rng.integers(0, 256, size=(n_units, cfg.n_freq, 2 * S, n_ant), dtype=np.uint8)
        w = rng.integers(-128, 128, size=(cfg.n_freq, n_ant, cfg.n_beams, 2), dtype=np.int8)
        bf = env.bfmod.Beamformer(cfg)
        stage = env.api.StokesBeams(bf, n_int)
        stage.set_weights(env.dev(w) if device_weights else w, STOKES_BEAMS)
        d_in = env.dev(packed)
        assert d_in.data_ptr() % 16 == 0
        if mode == 3:
            from test_gpu_cdd import _want_voltages

            want = _want_voltages(packed, w, STOKES_BEAMS)                     # complex64 [freq][k][pol][n_units * S]
            out = Out(env, (want.size * 2,), "int32", SENTINEL32)
            stage.voltages(d_in, n_units, out.t)
        else:
            want = so.stokes(packed, w, STOKES_BEAMS, n_int, so.geometry(cfg))   # int64 [unit][t][freq][k][4]
            assert stage.entries * n_units * 4 == want.size
            out = Out(env, want.shape, "int64", SENTINEL64)
            stage.compute(d_in, n_units, out.t)
        n = same_bits(out.read(), want, ("stokes", n_ant, mode))
        stage.close()
        bf.close()
        return n
    return run


def _stokes_rows():
    rows = []
    for (nks, vec), n_ant in sorted(STOKES_ANT.items()):
        for mode, what in sorted(STOKES_MODES.items()):
            rows.append(Row("stokes_kernel<%d, %s, %d>" % (nks, "true" if vec else "false", mode), "%d antennas, %s" % (n_ant, what), _stokes(n_ant, mode)))
    rows.append(Row("stokes_gather_kernel", "weights of 68 antennas from a device array, then the direct kernel", _stokes(68, 0, device_weights=True)))
    return rows


# ---- coherent dedispersion: cdd_kernel<log2 N, Stokes output> ------------------------------------------------------------------------
def _cdd(m, stokes):
    def run(env):
        import cdd_oracle as co
        from test_gpu_cdd import _full_scale, _random_table, _run_cdd

        n, n_edge = 1 << m, 1
        v = n - 2 * n_edge
        rng = np.random.default_rng(100 * m + stokes)
        table = _random_table(rng, 1, n)
        x = _full_scale(rng, (1, 1, 2, v + 1))                                  # two segments, the second one sample long
        y = co.dedisperse(x, table, n_edge)
        want = co.stokes(y, 1) if stokes else y
        bf = env.bfmod.Beamformer(env.cfg(n_ant=4, n_beams=4))
        stage = env.api.CoherentDedisperser(bf, 1, n, n_edge, table)
        assert stage.n_valid == v
        _run_cdd(env.torch, stage, x, 1 if stokes else 0, want, ("cdd", n, stokes))   # sentinels, guard words, bit for bit
        stage.close()
        bf.close()
        return want.size * (1 if stokes else 2)
    return run


def _cdd_rows():
    return [Row("cdd_kernel<%d, %s>" % (m, "true" if st else "false"), "N %d, 1 channel, K 1, n_edge 1, n_time V + 1, %s" % (1 << m, "Stokes n_int 1" if st else "voltages"),
                _cdd(m, st)) for m in range(6, 13) for st in (False, True)]


# ---- incoherent beam: incoherent_kernel<lanes per span, word> -----------------------------------------------------------------------
# (n_ant, n_pol, n_avg) -> span bytes: the smallest span of each (lanes, load width) class of tests/test_gpu_incoherent.py
IB_SHAPES = {(1, UINT4): (4, 2, 2), (1, UINT): (4, 1, 1), (4, UINT4): (64, 2, 1), (4, UINT): (20, 2, 1), (16, UINT4): (128, 2, 2), (16, UINT): (132, 1, 1),
             (64, UINT4): (256, 2, 16), (64, UINT): (516, 1, 5)}


def _ib(shape):
    def run(env):
        from test_gpu_incoherent import _check_shape

        small = shape[0] * shape[1] * shape[2] < 128
        # compact and as a column of a sentinel-filled detected array at beams 0, 5 and the last: four launches
        return 4 * _check_shape(env.torch, env.bfmod, np.random.default_rng(sum(shape)), shape, n_units=32 if small else 2, n_out=3 if shape == (4, 1, 1) else 2)
    return run


def _ib_rows():
    return [Row("incoherent_kernel<%d, %s>" % (lanes, word), "%d antennas, n_pol %d, n_avg %d: spans of %d bytes" % (s + (s[0] * s[1] * s[2],)), _ib(s))
            for (lanes, word), s in sorted(IB_SHAPES.items())]


# ---- correlator, voltage moments ---------------------------------------------------------------------------------------------------
def _corr(env):
    import corr_oracle

    cfg = env.cfg(n_ant=20, n_freq=3, n_out_per_gemm=3)                         # a ragged off-diagonal tile
    packed = np.random.default_rng(1).integers(0, 256, size=(2, 3, 6, 20), dtype=np.uint8)
    want = corr_oracle.visibilities(packed, 2)
    bf = env.bfmod.Beamformer(cfg)
    assert bf.corr_entries * 2 == want.size
    out = Out(env, want.shape, "int64", SENTINEL64)
    bf.correlate(env.dev(packed), 2, out.t)
    n = same_bits(out.read(), want, "corr")
    bf.close()
    return n


def _moments(n_ant):
    def run(env):
        import sk_oracle

        cfg = env.cfg(n_ant=n_ant, n_freq=3, n_out_per_gemm=3)
        packed = np.random.default_rng(n_ant).integers(0, 256, size=(2, 3, 6, n_ant), dtype=np.uint8)
        want = sk_oracle.moments(packed, 2)
        bf = env.bfmod.Beamformer(cfg)
        assert bf.sk_entries * 2 == want.size
        out = Out(env, want.shape, "int64", SENTINEL64)
        bf.voltage_moments(env.dev(packed), 2, out.t)
        n = same_bits(out.read(), want, ("moments", n_ant))
        bf.close()
        return n
    return run


# ---- gain solver, spatial null ---------------------------------------------------------------------------------------------------------
NAN_BITS = 0x7FF8DEADBEEF0001
INFO_FILL = 0x7F7F7F7F


def _cal_solve(resident):
    def run(env):
        import cal_oracle

        n_ant, n_freq, n_pol = 4, 3, 2
        rng = np.random.default_rng(7 + resident)
        vis, _ = cal_oracle.synth_vis(rng, n_ant, n_freq, n_pol, 2.0 ** 20, None, same_gains=False)
        want_g, want_i = cal_oracle.solve(vis, n_ant, model=None, flags=None, joint_pol=False)
        bf = env.bfmod.Beamformer(env.cfg(n_ant=n_ant, n_freq=n_freq, n_pol=n_pol, n_out_per_gemm=2))
        if not resident:
            bf.set_switch("cal_resident", 0)
        g, i = Out(env, (n_pol, n_freq, n_ant, 2), "int64", NAN_BITS), Out(env, (n_pol, n_freq, 2), "int32", INFO_FILL)
        bf.solve_gains(env.dev(vis), g.t, i.t, joint_pol=False)
        n = same_bits(i.read(), want_i.astype(np.int32), ("cal info", resident)) + same_bits(g.read(), np.ascontiguousarray(want_g, np.float64), ("cal gains", resident))
        bf.close()
        return n
    return run


def _calw(env):
    import cal_oracle

    n_freq, n_ant, n_beams = 2, 4, 8
    rng = np.random.default_rng(23)
    w = rng.integers(-128, 128, size=(n_freq, n_ant, n_beams, 2), dtype=np.int8)
    amp = rng.uniform(0.5, 1.5, size=(n_freq, n_ant))
    g = amp * np.exp(2j * np.pi * rng.uniform(size=amp.shape))
    gains = np.stack([g.real, g.imag], axis=-1)
    flags = np.array([0, 0, 1, 0], np.uint8)
    bf = env.bfmod.Beamformer(env.cfg(n_ant=n_ant, n_freq=n_freq, n_beams=n_beams, n_out_per_gemm=2))
    n = 0
    for mode, code in (("phase", cal_oracle.PHASE), ("full", cal_oracle.FULL)):
        want = cal_oracle.calibrate_weights(w, gains, flags, code)
        out = Out(env, w.shape, "int8", 0x7F)
        bf.calibrate_weights(env.dev(w), env.dev(gains), out.t, flags=env.dev(flags), mode=mode)
        n += same_bits(out.read(), want, ("calw", mode))
    bf.close()
    return n


def _null_solve(resident):
    def run(env):
        import null_oracle
        from test_gpu_null import _field

        n_ant, n_freq, n_pol, n_null = 4, 3, 2, 2
        rng = np.random.default_rng(11 + resident)
        vis = _field(rng, n_ant, n_freq, n_pol, 1, 20)
        wv, we, wi = null_oracle.solve(vis, n_ant, None, n_null=n_null, pol=-1)
        bf = env.bfmod.Beamformer(env.cfg(n_ant=n_ant, n_freq=n_freq, n_pol=n_pol, n_out_per_gemm=2))
        if not resident:
            bf.set_switch("null_resident", 0)
        v, e, i = (Out(env, (n_freq, n_null, n_ant, 2), "int64", NAN_BITS), Out(env, (n_freq, n_null + 1), "int64", NAN_BITS),
                   Out(env, (n_freq, 1 + 2 * n_null), "int32", INFO_FILL))
        bf.null_solve(env.dev(vis), v.t, e.t, i.t, n_null=n_null, pol=-1)
        n = (same_bits(i.read(), wi.astype(np.int32), ("null info", resident)) + same_bits(e.read(), np.ascontiguousarray(we, np.float64), ("null eig", resident)) +
             same_bits(v.read(), np.ascontiguousarray(wv, np.float64), ("null vectors", resident)))
        bf.close()
        return n
    return run


def _null_apply(env):
    import null_oracle
    from test_gpu_null import _signatures, _weights

    n_ant, n_beams, n_freq, n_null = 4, 8, 3, 2
    rng = np.random.default_rng(23)
    vis = null_oracle.exact_vis(_signatures(rng, 2, n_ant), [[3000.0, 0.0, 3000.0], [1500.0, 0.0, 0.0]], n_ant, n_freq, 1, noise=20, seed=12)
    w = _weights(rng, n_freq, n_ant, n_beams)
    vecs, eig, info = null_oracle.solve(vis, n_ant, None, n_null=n_null)
    bf = env.bfmod.Beamformer(env.cfg(n_ant=n_ant, n_pol=1, n_freq=n_freq, n_beams=n_beams, n_out_per_gemm=2))
    n = 0
    for mode, code in (("scaled", null_oracle.SCALED), ("clip", null_oracle.CLIP)):
        want_w, want_k = null_oracle.project(w, vecs, info, None, code)
        out, k = Out(env, w.shape, "int8", 0x7F), Out(env, (n_freq,), "int64", NAN_BITS)
        bf.null_weights(env.dev(w), env.dev(vecs), env.dev(info), out.t, n_null, mode=mode, scale=k.t)
        n += same_bits(out.read(), want_w, ("null weights", mode)) + same_bits(k.read(), np.ascontiguousarray(want_k, np.float64), ("null scale", mode))
    bf.close()
    return n


# ---- Faraday synthesis: rm_kernel<spectrum, peaks> -----------------------------------------------------------------------------------
def _rm(mode):
    def run(env):
        import rm_oracle as ro
        from test_gpu_rm import _random_table, _run

        n_rows, K, n_phi, n_chan = 2, 3, 17, 3
        rng = np.random.default_rng(5)
        rot, wn = _random_table(rng, n_phi, n_chan)
        s = rng.standard_normal((n_rows, n_chan, K, 4)).astype(np.float32)
        want = ro.synthesize(s, rot, wn, None)
        bf = env.bfmod.Beamformer(env.cfg(n_ant=4, n_beams=4))
        stage = env.api.FaradaySynthesis(bf, n_chan, n_phi, rot, wn)
        _run(env.torch, stage, s, None, want, ("rm", mode), mode)               # sentinels, guard words, bit for bit
        stage.close()
        bf.close()
        return (2 * want[0].size if mode != "peaks" else 0) + (8 * want[1].size if mode != "spec" else 0)
    return run


# ---- the stages behind the DM trials: search, periodicity search, folder, injector, conditioner, stamp cut ----------------------------------
def _sps(n_widths):
    def run(env):
        from sps_stage import run_stage
        from test_sps_cpu import series_for

        n_dm, n_t, n_beams = 2, 140, 4                                          # a whole tile of 128 times and a ragged one
        x = series_for(n_dm, n_t, n_beams, 50 + n_widths)
        bf = env.bfmod.Beamformer(env.bfmod.debug_config(n_beams=n_beams, n_freq=8))
        log = []
        run_stage(env.torch, bf, x, n_widths, [129, 11], 129, threshold=3.0, log=log)   # records to the bit against sps_oracle
        bf.close()
        return sum(rec["value"].size for _, rec, _ in log)
    return run


def _ffa(cfg, n_beams, n_dm, n_in, seed, detrend=None):
    """cfg = (tdec, n_seg, n_oct, p_lo, p_hi, K)."""
    def run(env):
        import ffa_detrend_stage
        import ffa_oracle
        import ffa_stage

        x = ffa_oracle.parity_input(seed, n_dm, n_in, n_beams)
        bf = env.bfmod.Beamformer(env.bfmod.debug_config(n_beams=n_beams, n_freq=8))
        log, sizes = [], [min(cfg[0] * cfg[1], 4096), 33]
        if detrend:
            ffa_detrend_stage.run_stage(env.torch, bf, x, cfg, detrend, sizes, 2, threshold=3.0, log=log)
        else:
            ffa_stage.run_stage(env.torch, bf, x, cfg, sizes, 2, threshold=3.0, log=log)   # records to the bit against ffa_oracle
        bf.close()
        assert log
        return sum(rec["value"].size + rec["shift"].size + rec["bin"].size for _, rec, _ in log)
    return run


def _ffa_rows():
    import ffa_stage

    rows = []
    for name in ("k1_p8", "k2_p8", "k3_p8", "k4_p16", "k5_p32", "k6_p64"):      # each K at the smallest p_lo it allows
        n_beams, n_dm, n_seg, p_lo, p_hi, tdec, n_oct, K, n_in, _, _ = ffa_stage.EDGE_CASES[name]
        rows.append(Row("ffa_search_kernel<%d>" % K, "%d beams, %d trials, n_seg %d, p %d .. %d" % (n_beams, n_dm, n_seg, p_lo, p_hi - 1),
                        _ffa(ffa_stage.case_cfg(name), n_beams, n_dm, n_in, sum(map(ord, name)))))
    rows.append(Row("ffa_decimate_kernel", "tdec 3 at n_seg 64: groups cut by the pushes", _ffa((3, 64, 1, 8, 11, 1), 4, 2, 64 * 3 * 2 + 7, 301)))
    rows.append(Row("ffa_octave_kernel", "two octaves at n_seg 64", _ffa((1, 64, 2, 8, 11, 1), 4, 2, 64 * 2 + 5, 302)))
    rows.append(Row("ffa_detrend_kernel", "blk 4, win 5 at n_seg 96", _ffa((1, 96, 1, 8, 13, 2), 4, 3, 96 * 2 + 5, 303, detrend=(4, 5))))
    return rows


def _psr(n_psr):
    def run(env):
        from test_gpu_psr import SIZES, bits, cuts_of, delays_for, models_for, order_matters, push_all, wide

        n_b, n_f, n_bins, n_rows = 4, 3, 5, 203
        rng = np.random.default_rng(4030 + n_psr)
        x = wide(rng, (n_rows, n_f, n_b))
        models, delays = models_for(n_psr, n_bins, n_rows, "fast"), delays_for(rng, n_psr, n_f, n_rows)
        want_prof, want_hits = order_matters(x, models, delays, n_bins)
        bf = env.bfmod.Beamformer(env.bfmod.debug_config(n_beams=n_b, n_freq=8))
        streams = [env.torch.cuda.Stream(), env.torch.cuda.Stream()]
        d_x = env.dev(x)
        env.torch.cuda.synchronize()
        folder = env.api.PulsarFolder(bf, n_f, 64, n_bins, models, delays)
        push_all(env.torch, folder, d_x, n_f * n_b * 4, cuts_of(n_rows, SIZES), streams)
        folder.dump()
        prof, hits, first_row, got_rows = folder.collect()
        assert (first_row, got_rows) == (0, n_rows) and np.array_equal(hits, want_hits)
        assert np.array_equal(bits(prof), bits(want_prof))
        folder.close()
        bf.close()
        return 2 * prof.size + hits.size
    return run


def _inj(kind, n):
    def run(env):
        import inj_cases
        from test_gpu_inj import run_case

        if kind == "burst":
            c = inj_cases.burst_case((4, 3, 7))                                 # its first two bursts overlap in cells; two more in front of them
            rng = np.random.default_rng(99)
            more = [(t0, rng.integers(0, 25, 3).astype(np.int32), inj_cases.wide(rng, (3, 7), 6), inj_cases.response_of(rng, 4)) for t0 in (20, 60)]
            c["bursts"] = (c["bursts"][:2] + more)[:n]                          # (every one inside the rows of the apply: one launch of n)
        else:
            c = inj_cases.train_case((4, 3, 5, n, "fast"))                      # n trains behind one burst
        want = inj_cases.expected(c)
        got = run_case(env.torch, env.bfmod, c, sizes=[inj_cases.N_ROWS])        # one apply: every pulse in one launch of its kind
        return same_bits(got, want, ("inj", kind, n))
    return run


def _cond(zero_dm):
    def run(env):
        import cond_oracle
        from test_gpu_cond import band, run_pushes

        n_b, n_f, window = 4, 3, 2
        x = band(np.random.default_rng(17 + zero_dm), 70, n_f, n_b)
        bf = env.bfmod.Beamformer(env.bfmod.debug_config(n_beams=n_b, n_freq=8))
        cond = env.api.Conditioner(bf, n_f, 33, baseline_pushes=window, zero_dm=zero_dm)
        orc = cond_oracle.Conditioner(n_f, n_b, window, zero_dm, 0.0, np.zeros(n_f, np.uint8))
        run_pushes(env.torch, env.hip, cond, orc, x, [33, 1, 32])               # a sentinel frame around every push's rows, bit for bit
        assert np.array_equal(cond.mask(), orc.mask)
        cond.close()
        bf.close()
        return x.size
    return run


def _stamp(env):
    import stamp_oracle as so
    from test_gpu_stamps import make_ladder, make_series

    n_f, n_b, n_dm, n_t, n_tau, tbin, fbin = 3, 4, 3, 40, 7, 2, 3
    delays = make_ladder(n_dm, n_f)
    series = make_series(31, n_t, n_f, n_b)
    bf = env.bfmod.Beamformer(env.bfmod.debug_config(n_beams=n_b, n_freq=8))
    dm = env.api.DmStream(bf, delays, n_f, 8, history_rows=n_t)
    d_series = env.dev(series)
    for at in range(0, n_t, 8):
        dm.push(d_series.data_ptr() + at * n_f * n_b * 4, 8)
    oldest, nxt, _ = dm.history()
    assert (oldest, nxt) == (0, n_t)
    reqs = [(0, 0, 0), (5, 2, 3), (n_t - n_tau * tbin - int(delays[1].max()), 1, 2), (n_t, 1, 1)]   # the last one: not pushed yet
    want, st_want = so.cut(series, delays, reqs, n_tau, tbin, fbin, oldest, nxt)
    assert list(st_want) == [0, 0, 0, 2]
    out = Out(env, want.shape, "int32", int(np.uint32(so.SENTINEL).view(np.int32)))
    st = dm.cut(reqs, n_tau, tbin, fbin, out.t)
    assert list(st) == list(st_want)
    n = same_bits(out.read(), want.view(np.int32), "stamp")
    dm.close()
    bf.close()
    return n


def _vcut(n_ant):
    def run(env):
        import vcut_oracle as vo
        from test_gpu_vcut import CAP, Cuts, _cfg, _units

        cfg = _cfg(env.bfmod, n_ant, 3, 1, 3)                                   # S 3, 3 channels; B = 2 n_ant bytes per sample
        S, n_units_out = 3, 1
        delays = np.array([[0, 0, 0], [0, 1, S + 1]], np.int32)
        units = _units(np.random.default_rng(n_ant), cfg, 4)
        d_units = env.dev(units)
        bf = env.bfmod.Beamformer(cfg)
        vh = env.api.VoltageHistory(bf, delays, CAP)
        for at in (0, 2):
            vh.push(d_units.data_ptr() + at * units[0].nbytes, 2)
        cuts = Cuts(env.torch, vh, units, delays)
        st = cuts.cut([(0, 0), (2, 1), (S + 1, 1), (4 * S, 0)], n_units_out, env.torch.cuda.Stream())   # guard bytes on both sides
        assert list(st) == [0, 0, 0, 2]
        cuts.compare()
        vh.close()
        bf.close()
        return 3 * n_units_out * units[0].nbytes // 4
    return run


def _rows():
    rows = _stokes_rows() + _cdd_rows() + _ib_rows()
    rows.append(Row("corr_kernel", "20 antennas, 3 channels, 2 units of 3 columns", _corr))
    rows.append(Row("moments_kernel<%s>" % UINT4, "16 antennas: 16-byte words", _moments(16)))
    rows.append(Row("moments_kernel<%s>" % UINT, "4 antennas: 4-byte words", _moments(4)))
    rows.append(Row("solve_kernel<true>", "4 antennas, visibilities resident in LDS", _cal_solve(True)))
    rows.append(Row("solve_kernel<false>", "4 antennas, switch cal_resident 0: re-read every iteration", _cal_solve(False)))
    rows.append(Row("calw_kernel", "4 antennas x 8 beams, both modes, a flagged antenna", _calw))
    rows.append(Row("null_solve_kernel<true>", "4 antennas, one interferer, resident in LDS", _null_solve(True)))
    rows.append(Row("null_solve_kernel<false>", "4 antennas, switch null_resident 0", _null_solve(False)))
    rows.append(Row("null_apply_kernel", "4 antennas x 8 beams, both modes", _null_apply))
    rows.append(Row("rm_kernel<true, true>", "2 rows, K 3, 17 depths, 3 channels: spectrum and peaks", _rm("both")))
    rows.append(Row("rm_kernel<false, true>", "the same: peaks only", _rm("peaks")))
    rows.append(Row("rm_kernel<true, false>", "the same: spectrum only", _rm("spec")))
    rows += [Row("sps_tile_kernel<%d>" % k, "%d widths, 2 trials x 140 times x 4 beams" % k, _sps(k)) for k in range(1, 9)]
    rows.append(Row("sps_finish_kernel", "behind the tiles of 3 widths", _sps(3)))
    rows += _ffa_rows()
    rows += [Row("psr_fold_kernel<%d>" % n, "%d pulsars, 4 beams, 3 channels, 5 bins" % n, _psr(n)) for n in range(1, 5)]
    rows += [Row("inj_burst_kernel<%d>" % n, "%d bursts in one apply" % n, _inj("burst", n)) for n in range(1, 5)]
    rows += [Row("inj_train_kernel<%d>" % n, "%d trains in one apply" % n, _inj("train", n)) for n in range(1, 5)]
    rows.append(Row("cond_totals_kernel", "4 beams, 3 channels, pushes of 33, 1 and 32 rows", _cond(True)))
    rows.append(Row("cond_summary_kernel", "the same", _cond(True)))
    rows.append(Row("cond_apply_kernel<true>", "the same: zero-DM on", _cond(True)))
    rows.append(Row("cond_apply_kernel<false>", "zero-DM off", _cond(False)))
    rows.append(Row("stamp_cut_kernel", "3 channels x 4 beams, 7 times of 2 rows, one band of 3 channels", _stamp))
    rows.append(Row("vcut_kernel<unsigned int __vector(4)>", "8 antennas: 16 bytes per sample", _vcut(8)))
    rows.append(Row("vcut_kernel<unsigned int>", "4 antennas: 8 bytes per sample", _vcut(4)))
    return rows


ROWS = _rows()
