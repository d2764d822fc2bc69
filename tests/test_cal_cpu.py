"""CPU checks of the gain solver (docs/CALIBRATION.md): the batched numpy oracle against an element-by-element Python restatement,
the association the oracle pins, the known answer, the exports' error convention without a handle, bf_cal_gain_entries, the Python
surface, the `beam -E / -G / -A / -P` command line and the gains file.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import cal_oracle  # noqa: E402

BEAM = os.path.join(ROOT, "dsabeamformer_amd", "beam")
BF_ERR_INVALID = -1


def _lib():
    from dsabeamformer_amd import _lib as l
    from dsabeamformer_amd import build as b

    b.build()
    return l.load()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _case(n, seed):
    """One noisy two-polarisation, two-channel field with a model and two flagged antennas whose rows hold garbage."""
    rng = np.random.default_rng(seed)
    ph = 2 * np.pi * rng.uniform(size=(2, n))
    model = np.stack([np.cos(ph), np.sin(ph)], axis=-1)
    vis, _ = cal_oracle.synth_vis(rng, n, 2, 1, model=model)                 # both polarisations see the same gains, each its own noise
    vis = np.repeat(vis, 2, axis=1) + rng.integers(-40, 41, size=(2, 2, vis.shape[2], 2))
    vis[:, :, [cal_oracle.bl(a, a) for a in range(n)], 1] = 0
    flags = np.zeros(n, np.uint8)
    flags[[0, n - 2]] = 1
    for a in (0, n - 2):                                                     # garbage wherever a flagged antenna takes part
        for b in range(n):
            vis[:, :, cal_oracle.bl(max(a, b), min(a, b))] = rng.integers(-2 ** 40, 2 ** 40, size=(2, 2, 2))
    return vis, model, flags


def test_the_batched_oracle_equals_the_per_element_restatement_and_pins_the_association():
    """n = 4 (less than a lane set) and n = 68 (the first second term of a lane), flags, a model, both polarisation modes: the same
    bits, the same iteration counts.  On that very case np.sum's association gives other bits somewhere -- without that, the bit
    comparison on the GPU would pin nothing."""
    other = 0
    for n, seed in ((4, 5), (68, 6)):
        vis, model, flags = _case(n, seed)
        for joint in (False, True):
            gains, info = cal_oracle.solve(vis, n, model=model, flags=flags, joint_pol=joint)
            assert gains.shape == (1 if joint else 2, 2, n, 2) and info.shape == (1 if joint else 2, 2, 2) and np.isfinite(gains).all()
            if n == 68:                                                      # (at n = 4 two antennas are left: only their product is determined)
                assert np.all(info[..., 1] == 1) and np.all(info[..., 0] % 2 == 0) and np.all(info[..., 0] <= 60), info.tolist()
            for po in range(gains.shape[0]):
                for f in range(2):
                    tri = vis[f].sum(axis=0) if joint else vis[f, po]
                    g, it, status = cal_oracle.solve_slow(tri, n, model[f], flags)
                    assert (it, status) == tuple(info[po, f]), (n, joint, po, f)
                    assert np.array_equal(_bits(np.array(g)), _bits(gains[po, f])), (n, joint, po, f)
            assert not gains[:, :, [0, n - 2]].any()                         # flagged: exactly zero
            # antenna 0 is flagged: the reference moved to 1, whose phase is zero to the rounding of the one complex product
            assert np.all(gains[:, :, 1, 0] > 0) and np.all(np.abs(gains[:, :, 1, 1]) <= 4 * 2.0 ** -52 * gains[:, :, 1, 0])
            plain, _ = cal_oracle.solve(vis, n, model=model, flags=flags, joint_pol=joint, summer=lambda t, axis: t.sum(axis))
            assert np.allclose(plain, gains, rtol=1e-9, atol=1e-9)
            other += int((_bits(plain) != _bits(gains)).sum())
        if n == 68:
            assert other > 0, "np.sum's order gave the same bits: the oracle pins no association"


def test_osum_is_the_written_order():
    rng = np.random.default_rng(3)
    for n in (1, 4, 63, 64, 65, 128, 200, 256):
        t = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, size=n)
        part = [0.0] * 64
        for i in range(n):
            part[i % 64] = part[i % 64] + float(t[i])
        for w in (32, 16, 8, 4, 2, 1):
            part = [part[i] + part[i + w] for i in range(w)]
        assert cal_oracle.osum(t).tobytes() == np.float64(part[0]).tobytes(), n
    assert cal_oracle.osum(np.full((3, 5), -0.0)).tobytes() == np.zeros(3).tobytes()   # the partial sums start from +0.0


def test_the_known_answer():
    """n = 4, every off-diagonal entry (2^20, 0), diagonal 2^20, no model: every gain is exactly (1024, 0) after two iterations."""
    vis = np.zeros((1, 1, 10, 2), np.int64)
    vis[..., 0] = 2 ** 20
    gains, info = cal_oracle.solve(vis, 4)
    assert np.array_equal(gains, np.tile([1024.0, 0.0], (1, 1, 4, 1))) and info.tolist() == [[[2, 1]]]
    g, it, status = cal_oracle.solve_slow(vis[0, 0], 4)
    assert g == [(1024.0, 0.0)] * 4 and (it, status) == (2, 1)


def test_the_weight_oracle_rounds_half_to_even_and_never_gives_minus_128():
    w = np.zeros((1, 4, 4, 2), np.int8)
    w[0, :, :, 0] = [[127, 1, 3, -128], [5, 7, -5, -127], [127, 127, 1, 2], [9, 9, 9, 9]]
    w[0, :, :, 1] = [[127, 0, 0, -128], [0, 0, 0, -128], [127, -127, 1, 2], [9, 9, 9, 9]]
    g = np.zeros((1, 4, 2))
    g[0] = [[np.sqrt(0.5), -np.sqrt(0.5)], [2.0, 0.0], [1.0, 0.0], [0.0, 0.0]]   # turn by +45 degrees; |g| 2 and 1: c = 0.5; zero gain
    ph = cal_oracle.calibrate_weights(w, g, mode=cal_oracle.PHASE)
    assert ph[0, 0, 0].tolist() == [0, 127]                                  # (127 + 127i) e^{i 45 deg} = 179.6i: clipped
    assert ph[0, 0, 3].tolist() == [0, -127] and ph.min() >= -127 and not ph[0, 3].any()
    assert np.array_equal(ph[0, 1], np.clip(w[0, 1], -127, 127)) and np.array_equal(ph[0, 2], w[0, 2])
    full = cal_oracle.calibrate_weights(w, g, mode=cal_oracle.FULL)          # k_f = min(1, 1, 2) = 1 (antenna 0 has |g| = 1 within rounding)
    k = min(np.sqrt(g[0, 0, 0] ** 2 + g[0, 0, 1] ** 2), 1.0)
    assert k == 1.0 or abs(k - 1.0) < 1e-15
    if k == 1.0:
        assert full[0, 1, :, 0].tolist() == [2, 4, -2, -64]                  # 2.5 -> 2, 3.5 -> 4, -2.5 -> -2: ties to even
    flagged = cal_oracle.calibrate_weights(w, g, flags=[0, 1, 0, 0], mode=cal_oracle.FULL)
    assert not flagged[0, 1].any() and flagged.min() >= -127


def test_every_new_export_refuses_a_null_handle():
    from dsabeamformer_amd._lib import BfCalOptions

    lib = _lib()
    opt = BfCalOptions()
    assert lib.bf_cal_default_options(C.byref(opt)) == 0
    assert (opt.tol, opt.max_iter, opt.ref_ant, opt.joint_pol) == (1e-10, 200, -1, 0)
    calls = [lambda: lib.bf_cal_default_options(None),
             lambda: lib.bf_solve_gains_device(None, None, None, None, C.byref(opt), None, None, None),
             lambda: lib.bf_solve_gains_device(None, None, None, None, None, None, None, None),
             lambda: lib.bf_calibrate_weights_device(None, None, None, None, 0, None, None)]
    for i, call in enumerate(calls):
        assert call() == BF_ERR_INVALID and lib.bf_last_error(), i


def test_gain_entries_at_c3_joint_and_not():
    from dsabeamformer_amd import api

    lib = _lib()
    c3 = api.production_config()
    assert (c3.n_ant, c3.n_pol, c3.n_freq) == (64, 2, 256)
    assert lib.bf_cal_gain_entries(C.byref(c3), 0) == 2 * 256 * 64 and lib.bf_cal_gain_entries(C.byref(c3), 1) == 256 * 64
    assert lib.bf_cal_gain_entries(None, 0) == 0


def test_python_surface_and_signature_table():
    from dsabeamformer_amd import _lib as l
    from dsabeamformer_amd import api, host

    names = ["bf_cal_default_options", "bf_cal_gain_entries", "bf_solve_gains_device", "bf_calibrate_weights_device"]
    assert all(n in l.SIGNATURES for n in names)
    assert l.SIGNATURES["bf_cal_gain_entries"] == (C.c_size_t, [C.POINTER(l.BfConfig), C.c_int])
    assert len(l.SIGNATURES["bf_solve_gains_device"][1]) == 8 and len(l.SIGNATURES["bf_calibrate_weights_device"][1]) == 7
    assert [f[0] for f in l.BfCalOptions._fields_] == ["tol", "max_iter", "ref_ant", "joint_pol"] and C.sizeof(l.BfCalOptions) == 24
    assert (l.BF_CAL_PHASE, l.BF_CAL_FULL) == (0, 1) == (cal_oracle.PHASE, cal_oracle.FULL)
    assert all(callable(getattr(api.Beamformer, m)) for m in ("solve_gains", "calibrate_weights", "gain_entries"))
    assert callable(host.read_gains_file) and callable(host.write_gains_file)


def test_beam_usage_errors_come_before_any_device():
    _lib()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    cases = [(["-G", "gains.bin"], "-G"),                                    # -G without -E
             (["-P"], "-P"),                                                 # -P without -E
             (["-E", "vis.bin"], "-G"),                                      # -E without -G
             (["-j", "27", "-E", "vis.bin", "-G", "gains.bin"], "-E"),       # -E with a run mode
             (["-k", "ring", "-E", "vis.bin", "-G", "gains.bin"], "-E"),
             (["-E", "vis.bin", "-G", "gains.bin", "-A", "other.bin"], "-A"),   # solve mode applies nothing
             (["-E", "/nonexistent/vis.bin", "-G", "gains.bin"], "vis.bin"),    # unreadable input: before any device
             (["-A", "/nonexistent/gains.bin"], "gains.bin")]
    for args, opt in cases:
        r = subprocess.run([BEAM] + args, capture_output=True, text=True, timeout=60, env=env, cwd=os.path.join(ROOT, "tests"))
        assert r.returncode != 0 and opt in r.stderr and "GPUassert" not in r.stderr and "Selected" not in r.stdout, (args, r.stderr)
    assert not os.path.exists(os.path.join(ROOT, "tests", "gains.bin"))      # and nothing was created


def test_a_gains_file_of_another_geometry_is_refused_before_any_device(tmp_path):
    from dsabeamformer_amd import host

    _lib()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    path = str(tmp_path / "gains.bin")
    host.write_gains_file(path, n_ant=32, n_pol=1, n_freq=256, first_channel=0,
                          records=[(0, 1, np.zeros((1, 256, 32, 2)), np.zeros((1, 256, 2), np.int32))])
    for args in (["-A", path], ["-j", "27", "-A", path]):
        r = subprocess.run([BEAM] + args, capture_output=True, text=True, timeout=60, env=env, cwd=str(tmp_path))
        assert r.returncode != 0 and "NANT" in r.stderr and "GPUassert" not in r.stderr and "Selected" not in r.stdout, (args, r.stderr)
    # a truncated file, a file of visibilities' kind, and the right geometry: the last one passes the check and stops at the missing device
    open(path, "ab").write(b"\0" * 5)
    r = subprocess.run([BEAM, "-A", path], capture_output=True, text=True, timeout=60, env=env, cwd=str(tmp_path))
    assert r.returncode != 0 and "gains.bin" in r.stderr and "GPUassert" not in r.stderr
    good = str(tmp_path / "good.bin")
    host.write_gains_file(good, n_ant=64, n_pol=1, n_freq=256, first_channel=0,
                          records=[(0, 1, np.ones((1, 256, 64, 2)), np.ones((1, 256, 2), np.int32))])
    r = subprocess.run([BEAM, "-A", good], capture_output=True, text=True, timeout=60, env=env, cwd=str(tmp_path))
    assert r.returncode != 0 and "-A" not in r.stderr and "GPUassert" in r.stderr, r.stderr


def test_extended_usage_lists_the_options():
    _lib()
    r = subprocess.run([BEAM, "-H"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and " -E vis_file -G gains_file [-P]" in r.stdout and " -A gains_file" in r.stdout and "gain solver" in r.stdout
    h = subprocess.run([BEAM, "-h"], capture_output=True, text=True, timeout=60)
    assert all(o not in h.stdout for o in ("-E", "-G", "-A ", "-P"))         # the reference's own text stays as it is


def test_the_gains_file_round_trip(tmp_path):
    from dsabeamformer_amd import host

    rng = np.random.default_rng(9)
    recs = [(7 * i, 4096 + i, rng.standard_normal((2, 3, 8, 2)), rng.integers(0, 200, size=(2, 3, 2)).astype(np.int32)) for i in range(3)]
    path = str(tmp_path / "gains.bin")
    host.write_gains_file(path, n_ant=8, n_pol=2, n_freq=3, first_channel=128, records=recs)
    assert os.path.getsize(path) == 4096 + 3 * (16 + 2 * 3 * 8 * 16 + 2 * 3 * 8)
    hdr, got = host.read_gains_file(path)
    assert hdr["CONTENT"] == "gains" and hdr["DTYPE"] == "float64" and hdr["LAYOUT"] == "pol,freq,ant,reim" and int(hdr["HDR_SIZE"]) == 4096
    assert (int(hdr["NANT"]), int(hdr["NPOL"]), int(hdr["NFREQ"]), int(hdr["FIRST_CHANNEL"])) == (8, 2, 3, 128)
    assert len(got) == 3
    for (b, c, g, i), (b2, c2, g2, i2) in zip(recs, got):
        assert (b, c) == (b2, c2) and np.array_equal(_bits(g), _bits(g2)) and np.array_equal(i, i2) and i2.dtype == np.int32
