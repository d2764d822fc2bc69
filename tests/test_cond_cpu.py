"""CPU-side checks of the conditioning stage (docs/CONDITIONING.md): the numpy oracle against a per-element restatement in Python
floats, the known answer, the scenario on the oracles alone, the new exports on NULL arguments, the ctypes table and the api
surface, and the `beam` driver's usage errors.  No GPU."""
import ctypes as C
import inspect
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import cond_oracle  # noqa: E402
import cond_scenario  # noqa: E402

BF_ERR_INVALID = -1
NEW_EXPORTS = ("bf_cond_default_options", "bf_cond_create", "bf_cond_destroy", "bf_cond_set_mask", "bf_cond_push", "bf_cond_mask_device",
               "bf_dm_stream_attach_conditioner")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the contract once more, element by element, in Python floats (IEEE doubles).  An fp32 operation is the double operation
# rounded to fp32: for +, -, *, / and sqrt on fp32 operands that double rounding is innocuous (53 >= 2 * 24 + 2).
def f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def plain_osum(v):
    p = [0.0] * 64
    for i, t in enumerate(v):
        p[i % 64] = p[i % 64] + t
    w = 32
    while w:
        for l in range(w):
            p[l] = p[l] + p[l + w]
        w //= 2
    return p[0]


def plain_median(v):
    return sorted(v)[(len(v) - 1) // 2]


def plain_conditioner(pushes, n_f, n_b, window, zero_dm, thr, static):
    """The outputs (nested lists [push][t][f][b]) and masks of the pushes (lists of rows [t][f][b] of Python floats)."""
    k = thr * 1.4826
    hist, outs, masks = [], [], []
    for rows in pushes:
        tot = {}
        for f in range(n_f):
            for b in range(n_b):
                S = Q = 0.0
                for s0 in range(0, len(rows), 32):
                    s = q = 0.0
                    for t in range(s0, min(s0 + 32, len(rows))):
                        s = s + rows[t][f][b]
                        q = q + rows[t][f][b] * rows[t][f][b]
                    S, Q = S + s, Q + q
                tot[f, b] = (S, Q)
        hist = (hist + [(len(rows), tot)])[-window:]
        n = float(sum(h[0] for h in hist))
        mu, var, mu32, r32 = {}, {}, {}, {}
        for f in range(n_f):
            for b in range(n_b):
                S = Q = 0.0
                for _, h in hist:
                    S, Q = S + h[f, b][0], Q + h[f, b][1]
                m = S / n
                v = Q / n - m * m
                mu[f, b], var[f, b], mu32[f, b] = m, v, f32(m)
                r32[f, b] = f32(1.0 / math.sqrt(v)) if v > (m * m) * 2.0 ** -40 else None      # None: dead
        cm = [plain_osum([mu[f, b] for b in range(n_b)]) / n_b for f in range(n_f)]
        cv = [plain_osum([max(var[f, b], 0.0) for b in range(n_b)]) / n_b for f in range(n_f)]
        mask = [bool(static[f]) or not (cm[f] > 0.0 and cv[f] > 0.0) for f in range(n_f)]
        if k > 0.0:
            elig = [f for f in range(n_f) if not mask[f]]
            if elig:
                q = {f: cv[f] / (cm[f] * cm[f]) for f in elig}
                med = plain_median(list(q.values()))
                mad = plain_median([abs(v - med) for v in q.values()])
                if mad > 0.0:
                    for f in elig:
                        if q[f] > med + k * mad:
                            mask[f] = True
        good = [f for f in range(n_f) if not mask[f]]
        inv = f32(1.0 / float(len(good))) if good else None
        out = []
        for row in rows:
            y = [[0.0 if mask[f] or r32[f, b] is None else f32(f32(row[f][b] - mu32[f, b]) * r32[f, b]) for b in range(n_b)] for f in range(n_f)]
            if zero_dm and good:
                for b in range(n_b):
                    z = 0.0
                    for f in good:
                        z = f32(z + y[f][b])
                    z = f32(z * inv)
                    for f in good:
                        y[f][b] = f32(y[f][b] - z)
            out.append(y)
        outs.append(out)
        masks.append([int(m) for m in mask])
    return outs, masks


def small_case():
    rng = np.random.default_rng(11)
    x = (rng.random((40, 3, 4)) * 1e3 * np.array([1.0, 7.0, 0.01])[None, :, None]).astype(np.float32)
    x[:, 1, 2] = np.float32(3.5)                        # a dead cell in a live channel
    return x


@pytest.mark.parametrize("zero_dm", [False, True])
def test_oracle_equals_the_elementwise_restatement(zero_dm):
    """n_freq 3, n_beams 4; a push of 33 rows (a whole segment and one row) and one of 7 behind it, window 2."""
    x = small_case()
    cuts = [(0, 33), (33, 7)]
    for thr, static in ((0.0, [0, 0, 0]), (0.5, [0, 0, 0]), (0.0, [0, 0, 1])):
        orc = cond_oracle.Conditioner(3, 4, 2, zero_dm, thr, static)
        outs, masks = plain_conditioner([[[[float(v) for v in fr] for fr in row] for row in x[a:a + n]] for a, n in cuts], 3, 4, 2, zero_dm, thr, static)
        for (a, n), out, mask in zip(cuts, outs, masks):
            got = orc.push(x[a:a + n])
            assert np.array_equal(bits(got), bits(np.array(out, np.float32))), (thr, static, a)
            assert list(orc.mask) == mask
        if not zero_dm:
            assert np.all(bits(got[:, 1, 2]) == 0)                                     # the dead cell: +0.0f stored


def test_the_segment_order_is_pinned_not_only_described():
    """On the 33-row case the totals in the contract's order differ in their bits from numpy's own association (np.sum along a
    contiguous axis adds in eight interleaved partial sums): an implementation that sums any other way is caught."""
    x = small_case()[:33]
    S, Q = cond_oracle.push_totals(x)
    x64 = np.ascontiguousarray(x.astype(np.float64).transpose(1, 2, 0))
    S2, Q2 = np.sum(x64, axis=-1), np.sum(x64 * x64, axis=-1)
    assert np.allclose(S, S2, rtol=1e-13) and np.allclose(Q, Q2, rtol=1e-13)
    assert np.any(S.view(np.uint64) != S2.view(np.uint64)) or np.any(Q.view(np.uint64) != Q2.view(np.uint64))
    # the same for OSUM against a left-to-right sum
    v = np.random.default_rng(2).random((5, 200))
    assert np.any(cond_oracle.osum(v).view(np.uint64) != np.cumsum(v, axis=-1)[:, -1].view(np.uint64))
    assert cond_oracle.lower_median([4.0, 1.0, 3.0, 2.0]) == 2.0 and cond_oracle.lower_median([5.0, 1.0, 3.0]) == 3.0


def test_known_answer():
    """n_beams 4, n_freq_total 2, one push of two rows: channel 0 is 1, 3 in every beam, channel 1 constant 5.  Channel 1 is dead and
    masked; channel 0 has mu 2, var 1: y = -1, +1.  With zero-DM, n_good = 1 and inv = 1: z = (+0.0f + y) * 1 = y, and y - z = +0.0f
    for both signs of y (x - x is +0 in round-to-nearest); the masked channel is the constant +0.0f.  Every output bit is 0."""
    x = np.zeros((2, 2, 4), np.float32)
    x[0, 0], x[1, 0], x[:, 1] = 1.0, 3.0, 5.0
    c = cond_oracle.Conditioner(2, 4, zero_dm=False)
    y = c.push(x)
    assert list(c.mask) == [0, 1] and c.n_good == 1
    assert np.array_equal(bits(y[:, 0]), bits(np.array([[-1.0] * 4, [1.0] * 4], np.float32))) and np.all(bits(y[:, 1]) == 0)
    c = cond_oracle.Conditioner(2, 4, zero_dm=True)
    y = c.push(x)
    assert list(c.mask) == [0, 1] and np.all(bits(y) == 0)


def test_scenario_on_the_oracles():
    """tests/support/cond_scenario.py: conditioned by the oracle, the mask is exactly {5, 17, 18}, the pulse is the strict maximum of
    all candidates at 1.5 x the best candidate that is not the pulse, and nothing that decides sits within 1e-6 of its bound; raw,
    the best candidate is a burst, not the pulse (what tests/test_gpu_cond.py asserts of the device's raw run)."""
    sc = cond_scenario
    x, d = sc.make()
    assert int(d.max()) == 18 and sc.chunk_sizes(d) == [30, 48, 48, 48, 48, 48]
    c = cond_oracle.Conditioner(sc.F, sc.B, sc.BASELINE_PUSHES, True, sc.AUTO_THRESHOLD)
    y = np.concatenate([c.push(x[k * sc.PUSH_ROWS:(k + 1) * sc.PUSH_ROWS]) for k in range(sc.N_PUSHES)])
    best = sc.check(sc.search(sc.dedisperse(y, d), d), d, c.mask)
    assert best[5] > 8.0
    raw = sc.search(sc.dedisperse(x, d), d)
    top = max(raw, key=lambda k: k[5])
    assert not sc.is_pulse(top, d) and top[0] in (68, 69, 70, 71)
    assert top[5] > 1.05 * max(k[5] for k in raw if sc.is_pulse(k, d))


@pytest.fixture(scope="module")
def lib():
    from dsabeamformer_amd import build as b
    from dsabeamformer_amd import _lib

    b.build()
    return _lib.load()


def test_new_exports_on_null_arguments(lib):
    from dsabeamformer_amd import _lib

    o = _lib.BfCondOptions(-1, -1, -1.0)
    lib.bf_cond_default_options(None)                    # (nothing to write to: returns)
    lib.bf_cond_default_options(C.byref(o))
    assert (o.baseline_pushes, o.zero_dm, o.auto_threshold) == (8, 1, 0.0)
    out = C.c_void_p(1)
    assert lib.bf_cond_create(None, 4, 4, C.byref(o), C.byref(out)) == BF_ERR_INVALID and not out.value
    assert b"NULL" in lib.bf_last_error()
    assert lib.bf_cond_create(None, 4, 4, C.byref(o), None) == BF_ERR_INVALID
    assert lib.bf_cond_destroy(None) == 0
    assert lib.bf_cond_set_mask(None, None) == BF_ERR_INVALID
    assert lib.bf_cond_push(None, None, 1, None) == BF_ERR_INVALID
    p = C.c_void_p()
    assert lib.bf_cond_mask_device(None, C.byref(p)) == BF_ERR_INVALID
    assert lib.bf_dm_stream_attach_conditioner(None, None) == BF_ERR_INVALID


def test_lib_table_and_api_surface():
    from dsabeamformer_amd import _lib, api

    for name in NEW_EXPORTS:
        assert name in _lib.SIGNATURES, name
    assert C.sizeof(_lib.BfCondOptions) == 16 and [f[0] for f in _lib.BfCondOptions._fields_] == ["baseline_pushes", "zero_dm", "auto_threshold"]
    sig = inspect.signature(api.Conditioner.__init__)
    assert list(sig.parameters) == ["self", "bf", "n_freq_total", "max_rows", "baseline_pushes", "zero_dm", "auto_threshold", "mask"]
    assert [sig.parameters[k].default for k in ("baseline_pushes", "zero_dm", "auto_threshold", "mask")] == [8, True, 0.0, None]
    assert list(inspect.signature(api.Conditioner.push).parameters) == ["self", "d_rows", "n_rows", "stream"]
    assert inspect.signature(api.Conditioner.push).parameters["stream"].default == 0
    for name in ("set_mask", "mask", "close"):
        assert callable(getattr(api.Conditioner, name))
    assert list(inspect.signature(api.DmStream.attach_conditioner).parameters) == ["self", "cond"]


def test_beam_usage_errors_and_extended_help(lib, tmp_path):
    """-n / -z / -U / -F without -M, -z / -U / -F without -n, an unreadable mask file and an index outside the band are usage errors
    before any device is touched (they read the same with and without a GPU); the options are listed under -H only."""
    from dsabeamformer_amd import build

    def beam(*args):
        return subprocess.run([build.BEAM] + [str(a) for a in args], capture_output=True, text=True, timeout=60)

    good = tmp_path / "mask.txt"
    good.write_text("# bad channels\n5\n 17  # the carrier\n\n18\n")
    outside = tmp_path / "outside.txt"
    outside.write_text("5\n256\n")
    junk = tmp_path / "junk.txt"
    junk.write_text("5x\n")
    for args, msg in ((("-j", 30, "-n", 3), "require the DM stage"), (("-j", 30, "-z"), "require the DM stage"), (("-j", 30, "-U", 5), "require the DM stage"),
                      (("-j", 30, "-F", good), "require the DM stage"),
                      (("-j", 30, "-M", 100, "-z"), "give -n"), (("-j", 30, "-M", 100, "-U", 5), "give -n"), (("-j", 30, "-M", 100, "-F", good), "give -n"),
                      (("-j", 30, "-M", 100, "-n", 0), "1 .. 64"), (("-j", 30, "-M", 100, "-n", 65), "1 .. 64"),
                      (("-j", 30, "-M", 100, "-n", 3, "-U", -1), ">= 0"),
                      (("-j", 30, "-M", 100, "-n", 3, "-F", tmp_path / "missing.txt"), "could not be read"),
                      (("-j", 30, "-M", 100, "-n", 3, "-F", outside), "not a channel index 0 .. 255"),
                      (("-j", 30, "-M", 100, "-n", 3, "-F", junk), "not a channel index")):
        r = beam(*args)
        assert r.returncode != 0 and msg in r.stderr and "GPUassert" not in r.stderr and "Selected:" not in r.stdout, (args, r.stderr)
    h, H = beam("-h"), beam("-H")
    assert H.returncode == 0 and "-n baseline_pushes [-z] [-U auto_threshold] [-F mask_file]" in H.stdout and "zero-DM" in H.stdout
    assert "baseline_pushes" not in h.stdout
