"""CPU checks of the voltage moments and the spectral-kurtosis flags (docs/SPECTRAL_KURTOSIS.md): the numpy oracle against a per-byte
Python loop and the known answer, bf_sk_select against the oracle's select to the bit (random moments, hand-built edges, the scene),
the exports' error convention without a handle or stage, bf_sk_entries, the Python surface, the `beam` command line (usage errors,
-H, select mode on a file the test writes) and the moments-file round trip.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import sk_oracle  # noqa: E402

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


@pytest.fixture(scope="module")
def scene_moments():
    """The scene (sk_oracle.scene: 16 antennas, 3 channels, 2 polarisations, 4096 columns per polarisation) and its moments; the
    oracle alone must flag exactly antennas 5, 9 and 12 and no channel before anything is compared with the library."""
    packed = sk_oracle.scene(20261019)
    mom = sk_oracle.moments(packed, 2)
    sk, cell, ant, chan = sk_oracle.select(mom, 4096)
    assert tuple(np.flatnonzero(ant)) == sk_oracle.SCENE_BAD and not chan.any(), (np.flatnonzero(ant), chan)
    assert np.all(cell[:, :, 5] == sk_oracle.LOW) and np.all(cell[:, :, 9] == sk_oracle.DEAD) and np.all(cell[:, :, 12] == sk_oracle.HIGH)
    return packed, mom


def _both(mom, M, **opt):
    """(library, oracle) results of one selection; sk must be bit-equal, the three flag arrays equal."""
    from dsabeamformer_amd import api

    _lib()
    got, want = api.sk_select(mom, M, **opt), sk_oracle.select(mom, M, **opt)
    assert got[0].dtype == np.float64 and np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)), (M, opt)
    for g, w, name in zip(got[1:], want[1:], ("cell", "ant_flags", "chan_flags")):
        assert g.dtype == np.uint8 and np.array_equal(g, w), (name, M, opt, g, w)
    return got


def test_oracle_equals_a_per_byte_loop_on_every_code():
    assert [(int(r), int(m)) for r, m in zip(sk_oracle.RE, sk_oracle.IM)] == [_nibbles(b) for b in range(256)]
    rng = np.random.default_rng(7)
    codes = np.concatenate([rng.permutation(256), rng.permutation(256)]).astype(np.uint8)   # every code, in [2][2][16 * 2][4]
    packed = codes.reshape(2, 2, 32, 4)
    got = sk_oracle.moments(packed, 2)
    want = np.zeros((2, 2, 4, 2), np.int64)
    for u in range(2):
        for f in range(2):
            for c in range(32):
                for a in range(4):
                    re, im = _nibbles(int(packed[u, f, c, a]))
                    p = re * re + im * im
                    want[f, c % 2, a] += (p, p * p)
    assert np.array_equal(got, want)
    assert int(sk_oracle.P.max()) == 128 and int(sk_oracle.P.min()) == 0


def test_the_known_answer():
    packed = np.frombuffer(sk_oracle.KNOWN_BYTES, np.uint8).reshape(1, 1, 4, 1)
    assert tuple(sk_oracle.moments(packed, 1)[0, 0, 0]) == sk_oracle.KNOWN == (236, 58 ** 2 + 29 ** 2 + 100 ** 2 + 49 ** 2)


def test_select_equals_the_oracle_on_random_moments():
    rng = np.random.default_rng(3)
    for n_freq, n_pol, n_ant, M in ((1, 1, 4, 2), (3, 2, 16, 4096), (5, 1, 20, 33), (2, 3, 8, 100000)):
        p = rng.integers(0, 129, size=(n_freq, n_pol, n_ant, 64))               # moments of 64 plausible samples, scaled to M
        mom = np.stack([p.sum(-1), (p * p).sum(-1)], axis=-1).astype(np.int64) * (M // 2)
        mom[rng.random(mom.shape[:3]) < 0.1] = 0                                 # some dead cells
        _both(mom, M)
        _both(mom, M, centre=0.9, n_sigma=3.0, max_bad_fraction_ant=0.25, max_bad_fraction_chan=0.1)


def test_select_edges():
    """Hand-built: a cell exactly on either bound is not flagged; s1 = 0; M = 2; every antenna flagged -> every channel flagged; the
    two fractions met exactly are not flagged."""
    # M = 4: scale = 5 / 3, half_width = n_sigma.  m1 = 4, m2 = 4 r: sk = (5 / 3) (r - 1).  r = 4 -> sk = 5 exactly; r = 1 -> sk = 0.
    M = 4
    assert (5.0 / 3.0) * (4.0 - 1.0) == 5.0
    mom = np.zeros((1, 1, 4, 2), np.int64)
    mom[0, 0, 0] = (4, 16)       # sk = 5.0 = centre + half_width with centre 1, n_sigma 4: on the upper bound
    mom[0, 0, 1] = (4, 4)        # sk = 0.0 = centre - half_width with centre 1, n_sigma 1: on the lower bound
    mom[0, 0, 2] = (4, 28)       # sk = 10: above
    mom[0, 0, 3] = (0, 0)        # dead
    sk, cell, ant, chan = _both(mom, M, centre=1.0, n_sigma=4.0)
    assert sk[0, 0].tolist() == [5.0, 0.0, 10.0, 0.0]
    assert cell[0, 0].tolist() == [0, 0, sk_oracle.HIGH, sk_oracle.DEAD]          # 5.0 > 5.0 is false; 0.0 < -3.0 is false
    sk, cell, ant, chan = _both(mom, M, centre=1.0, n_sigma=1.0)
    assert cell[0, 0].tolist() == [sk_oracle.HIGH, 0, sk_oracle.HIGH, sk_oracle.DEAD]   # 0.0 < 1.0 - 1.0 is false: on the lower bound
    sk, cell, ant, chan = _both(mom, M, centre=1.0, n_sigma=0.25)
    assert cell[0, 0].tolist() == [sk_oracle.HIGH, sk_oracle.LOW, sk_oracle.HIGH, sk_oracle.DEAD]
    assert ant.tolist() == [1, 1, 1, 1] and chan.tolist() == [1]                 # no good antenna: the channel is flagged
    # M = 2: scale = 3, half_width = n_sigma sqrt(2)
    m2 = np.zeros((2, 1, 4, 2), np.int64)
    m2[..., 0], m2[..., 1] = 10, 52                                              # r = 1.04
    sk, cell, ant, chan = _both(m2, 2)
    assert not cell.any() and not ant.any() and not chan.any()
    # the fractions met exactly: 4 channels x 1 polarisation; antenna 0 bad in 2 of 4 cells (0.5 * 4 = 2: not flagged), antenna 1 in 3
    # (flagged); 4 good antennas, 2 of them bad at channel 3 (0.5 * 4 = 2: not flagged), then a third
    mom = np.zeros((4, 1, 5, 2), np.int64)
    mom[..., 0], mom[..., 1] = 4096 * 8, 4096 * 128                              # r = 2, sk ~ 1
    mom[0:2, 0, 0] = 0                                                           # antenna 0: dead in 2 of 4
    mom[0:3, 0, 1] = 0                                                           # antenna 1: dead in 3 of 4 -> flagged
    mom[3, 0, 2] = 0                                                             # channel 3: antennas 2 and 3 bad, of 4 good
    mom[3, 0, 3] = 0
    sk, cell, ant, chan = _both(mom, 4096)
    assert ant.tolist() == [0, 1, 0, 0, 0] and chan.tolist() == [0, 0, 0, 0]
    mom[3, 0, 4] = 0                                                             # a third: 3 > 2
    sk, cell, ant, chan = _both(mom, 4096)
    assert ant.tolist() == [0, 1, 0, 0, 0] and chan.tolist() == [0, 0, 0, 1]


def test_select_on_the_scene(scene_moments):
    packed, mom = scene_moments
    sk, cell, ant, chan = _both(mom, 4096)
    assert tuple(np.flatnonzero(ant)) == sk_oracle.SCENE_BAD and not chan.any()
    half = 5.0 * 2.0 / 64.0
    assert (1.0 - half, 1.0 + half) == (0.84375, 1.15625)


def test_select_refuses_what_it_cannot_estimate():
    lib = _lib()
    mom = np.ones((1, 1, 4, 2), np.int64)
    p = mom.ctypes.data_as(C.c_void_p)
    for M in (0, 1):
        assert lib.bf_sk_select(p, M, 1, 1, 4, None, None, None, None, None) == BF_ERR_INVALID and lib.bf_last_error()
    assert lib.bf_sk_select(None, 4096, 1, 1, 4, None, None, None, None, None) == BF_ERR_INVALID
    assert lib.bf_sk_select(p, 2, 1, 1, 4, None, None, None, None, None) == 0    # every output is optional, the options too


def test_every_new_export_refuses_a_null_handle_or_stage():
    lib = _lib()
    out, n = C.c_void_p(), C.c_uint64()
    calls = [lambda: lib.bf_sk_device(None, None, 1, None, 0, None),
             lambda: lib.bf_sk_create(None, 2, C.byref(out)),
             lambda: lib.bf_sk_create(None, 2, None),
             lambda: lib.bf_sk_push(None, None, 1, None),
             lambda: lib.bf_sk_push_block(None, 0, 0, 0, 1),
             lambda: lib.bf_sk_dump(None, None),
             lambda: lib.bf_sk_collect(None, None, C.byref(n)),
             lambda: lib.bf_sk_pending(None),
             lambda: lib.bf_sk_default_options(None)]
    for i, call in enumerate(calls):
        assert call() == BF_ERR_INVALID and lib.bf_last_error(), i
    assert out.value is None
    assert lib.bf_sk_destroy(None) == 0                                          # like free(): nothing to destroy


def test_sk_entries_and_default_options():
    from dsabeamformer_amd import api
    from dsabeamformer_amd._lib import BfSkOptions

    lib = _lib()
    c3 = api.production_config()
    assert (c3.n_ant, c3.n_pol, c3.n_freq) == (64, 2, 256)
    assert lib.bf_sk_entries(C.byref(c3)) == 256 * 2 * 64
    assert lib.bf_sk_entries(C.byref(api.debug_config(n_ant=4, n_freq=3, n_pol=1))) == 3 * 4
    assert lib.bf_sk_entries(None) == 0
    o = BfSkOptions()
    assert lib.bf_sk_default_options(C.byref(o)) == 0
    assert (o.centre, o.n_sigma, o.max_bad_fraction_ant, o.max_bad_fraction_chan) == (1.0, 5.0, 0.5, 0.5)


def test_python_surface_and_signature_table():
    from dsabeamformer_amd import _lib as l
    from dsabeamformer_amd import api, host

    names = ["bf_sk_device", "bf_sk_entries", "bf_sk_default_options", "bf_sk_select", "bf_sk_create", "bf_sk_destroy", "bf_sk_push",
             "bf_sk_push_block", "bf_sk_dump", "bf_sk_collect", "bf_sk_pending"]
    assert all(n in l.SIGNATURES for n in names)
    assert l.SIGNATURES["bf_sk_entries"][0] is C.c_size_t and l.SIGNATURES["bf_sk_push_block"][1] == [C.c_void_p] + [C.c_int] * 4
    assert (l.BF_SK_DEAD, l.BF_SK_LOW, l.BF_SK_HIGH) == (sk_oracle.DEAD, sk_oracle.LOW, sk_oracle.HIGH) == (1, 2, 4)
    assert callable(api.Beamformer.voltage_moments) and isinstance(api.Beamformer.sk_entries, property)
    assert callable(api.sk_select) and callable(host.read_moments_file)
    assert all(callable(getattr(api.SpectralKurtosis, m)) for m in ("push", "push_block", "dump", "collect", "close"))
    assert isinstance(api.SpectralKurtosis.pending, property)


def _vis_header_only(path, n_ant):
    text = ("HDR_VERSION 1.0\nHDR_SIZE 4096\nINSTRUMENT DSA\nCONTENT visibilities\nDTYPE int64\nENDIAN little\nLAYOUT x\n"
            "RECORD_HEADER_BYTES 16\nNANT %d\nNPOL 1\nNFREQ 1\nFIRST_CHANNEL 0\n" % n_ant).encode()
    open(path, "wb").write(text.ljust(4096, b"\0"))


def test_beam_usage_errors_come_before_any_device(tmp_path, scene_moments):
    _lib()
    env = dict(os.environ, **NO_DEVICE)
    mom_file, vis_file, flags, far = (str(tmp_path / n) for n in ("m.bin", "vis.bin", "flags.txt", "far.txt"))
    sk_oracle.write_moments_file(mom_file, 0, [(0, 4096, scene_moments[1])])
    _vis_header_only(vis_file, 16)
    open(flags, "w").write("# antennas\n5\n9\n")
    open(far, "w").write("3\n16\n")                                              # 16 is outside [0, NANT)
    out = str(tmp_path / "out.txt")
    missing = str(tmp_path / "nothing_here")
    cases = [(["-Y", "m.bin"], "-Y"),                                            # the moments without the observation mode
             (["-j", "27", "-J", "2"], "-J"),                                    # -J without -Y
             (["-j", "27", "-Y", "m.bin", "-J", "0"], "-J"),                     # -J < 1
             (["-e", mom_file], "-O"),                                           # -e without -O
             (["-e", mom_file, "-O", out, "-j", "27"], "-e"),                    # -e together with a run, the solver or -A
             (["-e", mom_file, "-O", out, "-k", "ring"], "-e"),
             (["-e", mom_file, "-O", out, "-E", vis_file, "-G", "g.bin"], "-e"),
             (["-e", mom_file, "-O", out, "-A", "g.bin"], "-e"),
             (["-O", out], "-e"), (["-q", out], "-e"), (["-t", "3"], "-e"), (["-m", "0.9"], "-e"),   # select options without -e
             (["-f", flags], "-f"),                                              # -f without -E or -A
             (["-j", "27", "-f", flags], "-f"),
             (["-e", missing, "-O", out], "-e"),                                 # unreadable files
             (["-e", vis_file, "-O", out], "-e"),                                # (not a file of moments)
             (["-E", vis_file, "-G", "g.bin", "-f", missing], "-f"),
             (["-E", vis_file, "-G", "g.bin", "-f", far], "-f")]                 # an index outside [0, NANT)
    for args, opt in cases:
        r = subprocess.run([BEAM] + args, capture_output=True, text=True, timeout=60, env=env, cwd=str(tmp_path))
        assert r.returncode != 0 and opt in r.stderr and "GPUassert" not in r.stderr and "Selected" not in r.stdout, (args, r.stdout, r.stderr)
    assert not os.path.exists(out) and not os.path.exists(str(tmp_path / "g.bin"))   # and nothing was created
    assert sorted(os.listdir(str(tmp_path))) == ["far.txt", "flags.txt", "m.bin", "vis.bin"]


def test_extended_usage_lists_the_options():
    _lib()
    r = subprocess.run([BEAM, "-H"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for text in (" -Y file ", "-J sk_blocks", " -e moments_file ", "-O ant_file", "-q chan_file", "-t n_sigma", "-m centre", " -f ant_file "):
        assert text in r.stdout, text
    h = subprocess.run([BEAM, "-h"], capture_output=True, text=True, timeout=60)
    assert "-Y" not in h.stdout and "-J" not in h.stdout and "moments" not in h.stdout   # the reference's own text stays as it is


def test_moments_file_round_trip(tmp_path, scene_moments):
    from dsabeamformer_amd import host

    mom = scene_moments[1]
    path = str(tmp_path / "m.bin")
    sk_oracle.write_moments_file(path, 128, [(0, 100, mom), (3, 7, mom + 1)])
    hdr, dumps = host.read_moments_file(path)
    assert hdr["CONTENT"] == "voltage_moments" and hdr["DTYPE"] == "int64" and hdr["LAYOUT"] == "freq,pol,ant,m1m2"
    assert (int(hdr["NANT"]), int(hdr["NPOL"]), int(hdr["NFREQ"]), int(hdr["FIRST_CHANNEL"]), int(hdr["HDR_SIZE"])) == (16, 2, 3, 128, 4096)
    assert [(d[0], d[1]) for d in dumps] == [(0, 100), (3, 7)]
    assert np.array_equal(dumps[0][2], mom) and np.array_equal(dumps[1][2], mom + 1)
    assert os.path.getsize(path) == 4096 + 2 * (16 + mom.nbytes)


def _indices(path):
    lines = open(path).read().splitlines()
    assert lines and lines[0].startswith("#")
    return [int(x) for x in lines if x.strip() and not x.startswith("#")]


def test_beam_select_mode_sums_the_records(tmp_path, scene_moments):
    """`beam -e` on a file written here: two records that SUM to the scene (2048 columns each) give the scene's flag files; neither
    half alone decides.  -t and -m override the defaults as the oracle says; FIRST_CHANNEL offsets the channel indices."""
    _lib()
    packed, mom = scene_moments
    half = packed.shape[2] // 2
    a, b = sk_oracle.moments(packed[:, :, :half], 2), sk_oracle.moments(packed[:, :, half:], 2)
    assert np.array_equal(a + b, mom)
    path, ants, chans = (str(tmp_path / n) for n in ("m.bin", "ant.txt", "chan.txt"))
    sk_oracle.write_moments_file(path, 128, [(0, 2048, a), (1, 2048, b)])
    env = dict(os.environ, **NO_DEVICE)
    r = subprocess.run([BEAM, "-e", path, "-O", ants, "-q", chans], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and "Selected" not in r.stdout, r.stdout + r.stderr
    assert _indices(ants) == list(sk_oracle.SCENE_BAD) and _indices(chans) == []
    assert "4096 columns" in r.stdout and "3 of 16 antennas" in r.stdout
    # a centre of 0.5 and half a sigma: every live cell is HIGH -> every antenna, and then every channel, is flagged
    want = sk_oracle.select(mom, 4096, centre=0.5, n_sigma=0.5)
    r = subprocess.run([BEAM, "-e", path, "-O", ants, "-q", chans, "-t", "0.5", "-m", "0.5"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert _indices(ants) == np.flatnonzero(want[2]).tolist() and _indices(chans) == (128 + np.flatnonzero(want[3])).tolist()
    assert len(_indices(chans)) == 3
