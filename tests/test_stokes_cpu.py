"""CPU checks of the full-Stokes follow-up beams (docs/STOKES.md): the numpy oracle against a per-sample Python loop on every byte
code, the hand-computed known answer, the polarisation identities, the tie to the committed oracle (I at n_int = n_avg is the detected
power), bf_stokes_entries, the exports' error convention without a handle or stage, the Python surface, the `beam` command line
(usage errors, -H) and the file round trip.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import stokes_oracle as so  # noqa: E402

BEAM = os.path.join(ROOT, "dsabeamformer_amd", "beam")
BF_ERR_INVALID = -1
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")                # no device either way: nothing here may need one


def _lib():
    from dsabeamformer_amd import _lib as l
    from dsabeamformer_amd import build as b

    b.build()
    return l.load()


def _nibbles(b):
    re, im = b >> 4, b & 15
    return (re - 16 if re & 8 else re), (im - 16 if im & 8 else im)


def _loop(packed, w, beams, n_int, geom):
    """The contract sample by sample in Python integers."""
    S = geom.n_out_per_gemm * geom.n_avg
    n_units = packed.shape[0]
    out = np.zeros((n_units, S // n_int, geom.n_freq, len(beams), 4), np.int64)
    for u in range(n_units):
        for f in range(geom.n_freq):
            for k, b in enumerate(beams):
                for j in range(S):
                    n = []
                    for c in (2 * j, 2 * j + 1):
                        re = im = 0
                        for a in range(geom.n_ant):
                            vr, vi = _nibbles(int(packed[u, f, c, a]))
                            wr, wi = int(w[f, a, b, 0]), int(w[f, a, b, 1])
                            re += vr * wr - vi * wi
                            im += vi * wr + vr * wi
                        n.append((re, im))
                    (xr, xi), (yr, yi) = n
                    out[u, j // n_int, f, k] += (xr * xr + xi * xi + yr * yr + yi * yi, xr * xr + xi * xi - yr * yr - yi * yi,
                                                 2 * (xr * yr + xi * yi), 2 * (xi * yr - xr * yi))
    return out


def test_oracle_equals_a_per_sample_loop_on_every_code():
    assert [(int(r), int(m)) for r, m in zip(so.RE, so.IM)] == [_nibbles(b) for b in range(256)]
    rng = np.random.default_rng(7)
    geom = so.Geometry(n_ant=4, n_freq=2, n_out_per_gemm=3, n_avg=4, n_beams=5)  # S = 12: 2 units x 2 channels x 24 columns x 4 = 384 bytes
    codes = np.concatenate([rng.permutation(256), rng.integers(0, 256, 128)]).astype(np.uint8)
    packed = codes.reshape(2, 2, 24, 4)
    assert len(set(packed.ravel().tolist())) == 256
    w = rng.integers(-128, 128, size=(2, 4, 5, 2), dtype=np.int8)
    w[0, 0, 4], w[1, 3, 0] = (-128, -128), (-128, 127)
    for n_int, beams in ((1, [4, 0, 2]), (3, [1]), (4, [0, 1, 2, 3, 4]), (12, [3, 3])):
        got = so.stokes(packed, w, beams, n_int, geom)
        assert got.dtype == np.int64 and got.shape == (2, 12 // n_int, 2, len(beams), 4)
        assert np.array_equal(got, _loop(packed, w, beams, n_int, geom)), n_int


def test_the_known_answer():
    got = so.stokes(so.KNOWN_PACKED, so.KNOWN_WEIGHTS, [0], 1, so.KNOWN_GEOMETRY)
    assert got.shape == (1, 1, 1, 1, 4)
    assert tuple(int(v) for v in got[0, 0, 0, 0]) == so.KNOWN == (2775057, 636023, -2152472, -1631956)
    re, im = so.beam_samples(so.KNOWN_PACKED, so.KNOWN_WEIGHTS, [0])
    assert (re.ravel().tolist(), im.ravel().tolist()) == ([-808, 19], [1026, -1034])


def test_the_polarisation_identities():
    geom = so.Geometry(n_ant=8, n_freq=2, n_out_per_gemm=3, n_avg=2, n_beams=6)
    for n_int in (1, 2, 6):
        p, w = so.scene(11, geom, 2, "equal")
        s = so.stokes(p, w, [5, 0, 3], n_int, geom)
        assert s[..., 0].min() > 0 and not s[..., 1].any() and not s[..., 3].any() and np.array_equal(s[..., 2], s[..., 0])
        p, w = so.scene(12, geom, 2, "quarter")
        s = so.stokes(p, w, [5, 0, 3], n_int, geom)
        assert s[..., 0].min() > 0 and not s[..., 1].any() and not s[..., 2].any() and np.array_equal(s[..., 3], -s[..., 0])


def test_swapping_the_feeds_negates_q_and_v():
    geom = so.Geometry(n_ant=12, n_freq=3, n_out_per_gemm=2, n_avg=3, n_beams=4)
    p, w = so.scene(13, geom, 2)
    swapped = p.copy()
    swapped[:, :, 0::2], swapped[:, :, 1::2] = p[:, :, 1::2], p[:, :, 0::2]
    for n_int in (1, 3):
        a, b = so.stokes(p, w, [2, 1], n_int, geom), so.stokes(swapped, w, [2, 1], n_int, geom)
        assert a[..., 1].any() and a[..., 3].any()
        assert np.array_equal(a[..., 0], b[..., 0]) and np.array_equal(a[..., 2], b[..., 2])
        assert np.array_equal(a[..., 1], -b[..., 1]) and np.array_equal(a[..., 3], -b[..., 3])


def test_stokes_I_is_the_committed_oracles_power():
    """I at n_int = n_avg, times alpha^2, is oracle.beamform_exact of the same beams: the new oracle tied to the committed one."""
    import oracle as orc

    rng = np.random.default_rng(5)
    g = orc.Geom(n_beams=6, n_ant=20, n_freq=3, n_pol=2, n_avg=4, n_out_per_gemm=3)
    geom = so.Geometry(g.n_ant, g.n_freq, g.n_out_per_gemm, g.n_avg, g.n_beams)
    packed = rng.integers(0, 256, size=(2, g.n_freq, g.n_time, g.n_ant), dtype=np.uint8)
    w = rng.integers(-128, 128, size=(g.n_freq, g.n_ant, g.n_beams, 2), dtype=np.int8)
    beams = [4, 0, 5]
    s = so.stokes(packed, w, beams, g.n_avg, geom)                               # [u][o][f][k][4]
    a2 = np.float64(np.float32(1.0 / 127)) ** 2
    want = orc.beamform_exact(g, w, packed)[..., beams]                          # float64 [u][o][f][k]
    assert np.array_equal(a2 * s[..., 0].astype(np.float64), want)


def test_entries():
    from dsabeamformer_amd import api

    lib = _lib()
    c3 = api.production_config()
    assert lib.bf_stokes_entries(C.byref(c3), 4, 16) == 8 * 256 * 4
    assert lib.bf_stokes_entries(C.byref(c3), 16, 1) == 128 * 256 * 16 and lib.bf_stokes_entries(C.byref(c3), 1, 128) == 256
    for k, n_int in ((0, 16), (17, 16), (4, 0), (4, -1), (4, 3), (4, 256)):
        assert lib.bf_stokes_entries(C.byref(c3), k, n_int) == 0, (k, n_int)
    assert lib.bf_stokes_entries(None, 4, 16) == 0
    assert lib.bf_stokes_entries(C.byref(api.production_config(n_pol=1)), 4, 16) == 0


def test_every_new_export_refuses_a_null_handle_or_stage():
    lib = _lib()
    out, n = C.c_void_p(), C.c_int()
    beams = (C.c_int * 1)(0)
    calls = [lambda: lib.bf_stokes_create(None, 1, 2, C.byref(out)),
             lambda: lib.bf_stokes_create(None, 1, 2, None),
             lambda: lib.bf_stokes_set_weights(None, None, beams, 1),
             lambda: lib.bf_stokes_set_weights_device(None, None, beams, 1, None),
             lambda: lib.bf_stokes_device(None, None, 1, None, None),
             lambda: lib.bf_stokes_push(None, None, 1, None),
             lambda: lib.bf_stokes_push_block(None, 0, 0, 0, 1),
             lambda: lib.bf_stokes_collect(None, None, C.byref(n)),
             lambda: lib.bf_stokes_pending(None)]
    for i, call in enumerate(calls):
        assert call() == BF_ERR_INVALID and lib.bf_last_error(), i
    assert out.value is None
    assert lib.bf_stokes_destroy(None) == 0                                      # like free(): nothing to destroy


def test_python_surface_and_signature_table():
    from dsabeamformer_amd import _lib as l
    from dsabeamformer_amd import api, host

    names = ["bf_stokes_entries", "bf_stokes_create", "bf_stokes_destroy", "bf_stokes_set_weights", "bf_stokes_set_weights_device",
             "bf_stokes_device", "bf_stokes_push", "bf_stokes_push_block", "bf_stokes_collect", "bf_stokes_pending"]
    assert all(n in l.SIGNATURES for n in names)
    assert l.SIGNATURES["bf_stokes_entries"][0] is C.c_size_t and l.SIGNATURES["bf_stokes_push_block"][1] == [C.c_void_p] + [C.c_int] * 4
    assert l.BF_STOKES_MAX_BEAMS == 16
    for member in ("set_weights", "compute", "push", "push_block", "collect", "close"):
        assert callable(getattr(api.StokesBeams, member)), member
    assert isinstance(api.StokesBeams.pending, property) and isinstance(api.StokesBeams.entries, property)
    assert callable(host.read_stokes_file) and host.STOKES_LAYOUT == "unit,time,freq,beam,iquv"


def test_beam_usage_errors_come_before_any_device(tmp_path):
    _lib()
    env = dict(os.environ, **NO_DEVICE)
    x = str(tmp_path / "s.bin")
    many = ",".join(str(b) for b in range(17))
    cases = [(["-x", x, "-b", "3"], "-x"),                                       # -x without -j / -k
             (["-j", "27", "-x", x], "-b"),                                      # -x without -b
             (["-j", "27", "-b", "3"], "-x"),                                    # -b without -x
             (["-j", "27", "-l", "4"], "-x"),                                    # -l without -x
             (["-j", "27", "-x", x, "-b", "3,256"], "256"),                      # a beam outside [0, n_beams)
             (["-j", "27", "-x", x, "-b", "-1"], "-1"),
             (["-j", "27", "-x", x, "-b", many], "16"),                          # more than 16 beams
             (["-j", "27", "-x", x, "-b", "3,17,3"], "twice"),                   # a duplicate
             (["-j", "27", "-x", x, "-b", "3,x"], "-b"),
             (["-j", "27", "-x", x, "-b", "3,"], "-b"),
             (["-j", "27", "-x", x, "-b", "3", "-l", "0"], "-l"),                # -l < 1
             (["-j", "27", "-x", x, "-b", "3", "-l", "-2"], "-l"),
             (["-j", "27", "-x", x, "-b", "3", "-l", "3"], "-l")]                # 3 does not divide 8 * 16
    for args, word in cases:
        r = subprocess.run([BEAM] + args, capture_output=True, text=True, timeout=60, env=env, cwd=str(tmp_path))
        assert r.returncode != 0 and r.stderr.startswith("beam: ") and word in r.stderr and "GPUassert" not in r.stderr, (args, r.stdout, r.stderr)
        assert "Selected" not in r.stdout and "hip" not in r.stderr.lower(), (args, r.stdout, r.stderr)
    assert os.listdir(str(tmp_path)) == []                                       # and nothing was created


def test_extended_usage_lists_the_options():
    _lib()
    r = subprocess.run([BEAM, "-H"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for text in (" -x file ", "-b b0,b1,...", "[-l n_int]"):
        assert text in r.stdout, text
    h = subprocess.run([BEAM, "-h"], capture_output=True, text=True, timeout=60)
    assert "-x" not in h.stdout and "Stokes" not in h.stdout                     # the reference's own text stays as it is


def test_stokes_file_round_trip(tmp_path):
    from dsabeamformer_amd import host

    geom = so.Geometry(n_ant=8, n_freq=3, n_out_per_gemm=2, n_avg=4, n_beams=300)
    rng = np.random.default_rng(3)
    beams, n_int = [255, 3, 17], 2
    records = [(0, rng.integers(-2 ** 62, 2 ** 62, size=(4, 4, 3, 3, 4))), (4, rng.integers(-2 ** 62, 2 ** 62, size=(1, 4, 3, 3, 4)))]
    path = str(tmp_path / "s.bin.1")
    so.write_stokes_file(path, geom, 128, beams, n_int, records)
    hdr, got = host.read_stokes_file(path)
    assert hdr["CONTENT"] == "stokes" and hdr["DTYPE"] == "int64" and hdr["LAYOUT"] == "unit,time,freq,beam,iquv"
    assert hdr["BEAMS"] == beams and (int(hdr["NINT"]), int(hdr["NSEL"]), int(hdr["FIRST_CHANNEL"])) == (2, 3, 128)
    assert (int(hdr["NANT"]), int(hdr["NFREQ"])) == (8, 3)
    assert [(r[0], r[1]) for r in got] == [(0, 4), (4, 1)]
    for (first, data), r in zip(records, got):
        assert r[2].dtype == np.int64 and np.array_equal(r[2], data), first
