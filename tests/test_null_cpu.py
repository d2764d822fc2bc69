"""CPU checks of the spatial null (docs/NULLING.md): the batched numpy oracle against an element-by-element Python restatement, the
association the oracle pins, the known answers, the use rule at its edges, the projection's ties and clipping, the exports' error
convention without a handle, bf_null_vec_entries, the Python surface, the `beam -E / -Z / -y` command line and the null file.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import cal_oracle  # noqa: E402
import null_oracle  # noqa: E402

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
    """Two channels and two polarisations: two interferers plus noise in channel 0, noise alone in channel 1; two flagged antennas whose
    rows hold garbage."""
    rng = np.random.default_rng(seed)
    sig = np.exp(2j * np.pi * rng.uniform(size=(2, n)))
    vis = null_oracle.exact_vis(sig, [[3000.0, 0.0], [1000.0, 0.0]], n, 2, 2, noise=20, seed=seed + 1)
    vis[:, 1] += rng.integers(-5, 6, size=vis[:, 1].shape)                   # the polarisations differ
    vis[:, :, [cal_oracle.bl(a, a) for a in range(n)], 1] = 0
    flags = np.zeros(n, np.uint8)
    flags[[0, n - 2]] = 1
    for a in (0, n - 2):
        for b in range(n):
            vis[:, :, cal_oracle.bl(max(a, b), min(a, b))] = rng.integers(-2 ** 40, 2 ** 40, size=(2, 2, 2))
    return vis, flags


def test_the_batched_oracle_equals_the_per_element_restatement_and_pins_the_association():
    """n = 4 (less than a lane set) and n = 68 (the first second term of a lane), flags, n_null 1, 2 and 4, pol -1 and 1: the same bits,
    the same iteration counts and statuses.  On that very case np.sum's association gives other bits somewhere -- without that, the bit
    comparison on the GPU would pin nothing."""
    other = 0
    for n, seed in ((4, 5), (68, 6)):
        vis, flags = _case(n, seed)
        for n_null in (1, 2, 4):
            for pol in (-1, 1):
                vecs, eig, info = null_oracle.solve(vis, n, flags, n_null=n_null, pol=pol)
                assert vecs.shape == (2, n_null, n, 2) and eig.shape == (2, n_null + 1) and info.shape == (2, 1 + 2 * n_null)
                assert np.isfinite(vecs).all() and np.isfinite(eig).all() and not vecs[:, :, [0, n - 2]].any()
                for f in range(2):
                    tri = vis[f].sum(axis=0) if pol < 0 else vis[f, pol]
                    sv, se, si = null_oracle.solve_slow(tri, n, flags, n_null=n_null)
                    assert si == info[f].tolist(), (n, n_null, pol, f, si, info[f].tolist())
                    assert np.array_equal(_bits(np.array(se)), _bits(eig[f])) and np.array_equal(_bits(np.array(sv)), _bits(vecs[f])), (n, n_null, pol, f)
                if n == 68:
                    assert info[0, 0] == min(n_null, 2) and info[1, 0] == 0, info.tolist()
                    assert info[0, 2] == 1 and info[1, 2] == 0                # the interferer converges, the noise does not
                    for j in range(info[0, 0]):                              # x is Hermitian positive semidefinite: unit vectors, positive lambdas,
                        u = vecs[0, j, :, 0] + 1j * vecs[0, j, :, 1]         # and the iterate kept the phase of the start column
                        assert abs(np.vdot(u, u) - 1) < 1e-12 and eig[0, j] > 0
                plain = null_oracle.solve(vis, n, flags, n_null=n_null, pol=pol, summer=lambda t, axis: t.sum(axis))
                assert np.array_equal(plain[2][:, 0], info[:, 0])
                other += int((_bits(plain[0]) != _bits(vecs)).sum()) + int((_bits(plain[1]) != _bits(eig)).sum())
        if n == 68:
            assert other > 0, "np.sum's order gave the same bits: the oracle pins no association"


def test_the_known_answers():
    """n = 4, V = (2^20, 0) everywhere: u_0 = (0.5, 0) for every antenna, lambda_0 = 2^22 exactly, status 1 after the first multiplication,
    rest_0 = 0 so the vector is used (whatever min_ratio).  The same plus 2^20 on the diagonal: lambda_0 = 5 * 2^20, rest_0 = 2^20; used
    at min_ratio 4 and not at 6."""
    vis = np.zeros((1, 1, 10, 2), np.int64)
    vis[..., 0] = 2 ** 20
    for min_ratio in (4.0, 1e300):
        vecs, eig, info = null_oracle.solve(vis, 4, min_ratio=min_ratio)
        assert np.array_equal(vecs, np.tile([0.5, 0.0], (1, 1, 4, 1))) and eig.tolist() == [[2.0 ** 22, 2.0 ** 22]] and info.tolist() == [[1, 1, 1]]
    sv, se, si = null_oracle.solve_slow(vis[0, 0], 4)
    assert sv == [[(0.5, 0.0)] * 4] and se == [2.0 ** 22, 2.0 ** 22] and si == [1, 1, 1]
    vis[0, 0, [cal_oracle.bl(a, a) for a in range(4)], 0] += 2 ** 20
    for min_ratio, n_used in ((4.0, 1), (6.0, 0)):
        vecs, eig, info = null_oracle.solve(vis, 4, min_ratio=min_ratio)
        assert info[0, 0] == n_used and info[0, 2] == 1 and eig[0, 1] == 8 * 2.0 ** 20
        assert abs(eig[0, 0] / 2 ** 20 - 5) < 1e-9                           # (tr - lambda_0) / 3 = 2^20: the ratio is 5
        if n_used:
            assert np.allclose(vecs[0, 0], [0.5, 0.0], atol=1e-6)
        else:
            assert not vecs.any()


def test_the_use_rule_at_its_edges():
    """m = j + 1: with two unflagged antennas the second vector is never used, with one none is; rest <= 0 (an exact rank-one matrix):
    used at any min_ratio; min_ratio 0: every vector with lambda > 0 is used, noise included; a zero matrix: lambda = 0, never used."""
    rng = np.random.default_rng(3)
    n = 8
    sig = np.exp(2j * np.pi * rng.uniform(size=(1, n)))
    noisy = null_oracle.exact_vis(sig, [[3000.0]], n, 1, 1, noise=20, seed=4)
    two, one = np.ones(n, np.uint8), np.ones(n, np.uint8)
    two[[2, 5]] = 0
    one[2] = 0
    for min_ratio in (0.0, 4.0):
        assert null_oracle.solve(noisy, n, two, n_null=2, min_ratio=min_ratio)[2][0, 0] <= 1
        v, e, i = null_oracle.solve(noisy, n, one, n_null=2, min_ratio=min_ratio)
        assert i[0, 0] == 0 and not v.any() and np.isfinite(e).all()
    assert null_oracle.solve(noisy, n, two, n_null=2, min_ratio=0.0)[2][0, 0] == 1
    v, e, i = null_oracle.solve(noisy, n, n_null=4, min_ratio=0.0)
    assert i[0, 0] == 4 and np.all(e[0, :4] > 0)
    assert null_oracle.solve(noisy, n, n_null=4)[2][0, 0] == 1
    exact = np.zeros((1, 1, 16 * 17 // 2, 2), np.int64)
    exact[..., 0] = 2 ** 20                                                  # rank one on 16 antennas, u = 0.25: every sum exact, rest_0 = 0
    assert null_oracle.solve(exact, 16, min_ratio=1e300)[2].tolist() == [[1, 1, 1]]
    v, e, i = null_oracle.solve(np.zeros_like(exact), 16, n_null=2, min_ratio=0.0)
    assert i.tolist() == [[0, 0, 2, 0, 2]] and not v.any() and not e.any()


def test_the_projection_rounds_half_to_even_and_clips_in_both_modes():
    """u = (0.5, 0) on four antennas (the known answer).  w = (2, 0, 0, 0): c = 1, w' = (1.5, -0.5, -0.5, -0.5) -> (2, 0, 0, 0) by ties to
    even.  w = (127, -127, -127, -127): c = -127, w' = (190.5, -63.5, -63.5, -63.5): BF_NULL_CLIP gives (127, -64, -64, -64), BF_NULL_SCALED
    k = 127 / 190.5 = 2 / 3 and (127, -42, -42, -42).  A channel with n_used = 0 is copied, -128 included; a flagged antenna is zero."""
    vecs = np.zeros((2, 1, 4, 2))
    vecs[:, 0, :, 0] = 0.5
    info = np.array([[1, 1, 1], [0, 200, 0]], np.int32)
    w = np.zeros((2, 4, 4, 2), np.int8)
    w[0, 0, 0, 0] = 2
    w[0, :, 1, 0] = (127, -127, -127, -127)
    w[0, :, 2, 1] = (127, -127, -127, -127)                                  # the same in the imaginary parts
    w[0, :, 3] = (3, -128)
    w[1] = -128
    clip, k_clip = null_oracle.project(w[:, :, :2], vecs, info, mode=null_oracle.CLIP)
    assert clip[0, :, 0, 0].tolist() == [2, 0, 0, 0] and clip[0, :, 1, 0].tolist() == [127, -64, -64, -64] and k_clip.tolist() == [1.0, 1.0]
    out, k, wf = null_oracle.project(w, vecs, info, mode=null_oracle.SCALED, return_float=True)
    assert wf[0, :, 1, 0].tolist() == [190.5, -63.5, -63.5, -63.5] and wf[0, :, 2, 1].tolist() == [190.5, -63.5, -63.5, -63.5]
    assert k[1] == 1.0 and np.array_equal(out[1], w[1])                      # n_used = 0: byte for byte
    big = np.abs(wf[0]).max()
    assert k[0] == 127.0 / big and np.array_equal(out[0, :, :, 0], np.clip(np.rint(k[0] * wf[0, :, :, 0]), -127, 127).astype(np.int8))
    small = w[:, :, :3].copy()
    small[0, :, 2] = 0
    out, k = null_oracle.project(small, vecs, info, mode=null_oracle.SCALED)
    assert k[0] == 127.0 / 190.5 and out[0, :, 1, 0].tolist() == [127, -42, -42, -42] and out[0, :, 0, 0].tolist() == [1, 0, 0, 0]
    flagged, _ = null_oracle.project(w, vecs, info, flags=[0, 1, 0, 0], mode=null_oracle.CLIP)
    assert not flagged[:, 1].any() and np.array_equal(flagged[1, [0, 2, 3]], w[1, [0, 2, 3]]) and flagged[0].min() >= -127


def test_the_projected_weights_are_orthogonal_to_the_vectors_before_quantisation():
    """u_j^T w' = 0 to fp64 rounding: |u^T w'| <= 64 eps |w| |u| per beam (n = 68 terms of magnitude <= 127 sqrt(2) |u_a|, twice)."""
    vis, flags = _case(68, 6)
    vecs, eig, info = null_oracle.solve(vis, 68, flags, n_null=2)
    assert info[0, 0] == 2
    rng = np.random.default_rng(8)
    w = rng.integers(-127, 128, size=(2, 68, 12, 2), dtype=np.int8)
    _, _, wf = null_oracle.project(w, vecs, info, flags, return_float=True)
    wc = wf[0, :, :, 0] + 1j * wf[0, :, :, 1]
    for j in range(2):
        u = vecs[0, j, :, 0] + 1j * vecs[0, j, :, 1]
        assert np.abs(u @ wc).max() <= 64 * 2.0 ** -52 * 127 * np.sqrt(2 * 68), np.abs(u @ wc).max()
    assert np.array_equal(wf[1], np.where(flags[:, None, None] != 0, 0, w[1]).astype(np.float64))


def test_every_new_export_refuses_a_null_handle():
    from dsabeamformer_amd._lib import BfNullOptions

    lib = _lib()
    opt = BfNullOptions()
    assert lib.bf_null_default_options(C.byref(opt)) == 0
    assert (opt.n_null, opt.min_ratio, opt.tol, opt.max_iter, opt.pol) == (1, 4.0, 1e-6, 200, -1)
    calls = [lambda: lib.bf_null_default_options(None),
             lambda: lib.bf_null_solve_device(None, None, None, C.byref(opt), None, None, None, None),
             lambda: lib.bf_null_solve_device(None, None, None, None, None, None, None, None),
             lambda: lib.bf_null_weights_device(None, None, None, None, 1, None, 0, None, None, None)]
    for i, call in enumerate(calls):
        assert call() == BF_ERR_INVALID and lib.bf_last_error(), i


def test_vec_entries_at_c3_and_for_refused_arguments():
    from dsabeamformer_amd import api

    lib = _lib()
    c3 = api.production_config()
    assert (c3.n_ant, c3.n_pol, c3.n_freq) == (64, 2, 256)
    assert [lib.bf_null_vec_entries(C.byref(c3), k) for k in (1, 2, 4)] == [256 * 64, 2 * 256 * 64, 4 * 256 * 64]
    assert lib.bf_null_vec_entries(C.byref(c3), 0) == 0 and lib.bf_null_vec_entries(C.byref(c3), 5) == 0 and lib.bf_null_vec_entries(None, 1) == 0


def test_python_surface_and_signature_table():
    from dsabeamformer_amd import _lib as l
    from dsabeamformer_amd import api, host

    names = ["bf_null_default_options", "bf_null_vec_entries", "bf_null_solve_device", "bf_null_weights_device", "bfh_run_debug_observation4"]
    assert all(n in l.SIGNATURES for n in names)
    assert l.SIGNATURES["bf_null_vec_entries"] == (C.c_size_t, [C.POINTER(l.BfConfig), C.c_int])
    assert len(l.SIGNATURES["bf_null_solve_device"][1]) == 8 and len(l.SIGNATURES["bf_null_weights_device"][1]) == 10
    assert [f[0] for f in l.BfNullOptions._fields_] == ["min_ratio", "tol", "n_null", "max_iter", "pol"] and C.sizeof(l.BfNullOptions) == 32
    assert (l.BF_NULL_SCALED, l.BF_NULL_CLIP, l.BF_NULL_MAX) == (0, 1, 4) == (null_oracle.SCALED, null_oracle.CLIP, null_oracle.MAX_NULL)
    assert all(callable(getattr(api.Beamformer, m)) for m in ("null_solve", "null_weights", "null_vec_entries"))
    assert callable(host.read_null_file) and callable(host.write_null_file)


def _null_file(host, path, n_ant, n_freq, first_channel=0, n_null=1):
    host.write_null_file(path, n_ant=n_ant, n_freq=n_freq, first_channel=first_channel, n_null=n_null,
                         records=[(0, 1, np.zeros((n_freq, n_null, n_ant, 2)), np.zeros((n_freq, n_null + 1)),
                                   np.zeros((n_freq, 1 + 2 * n_null), np.int32))])


def test_beam_usage_errors_come_before_any_device(tmp_path):
    from dsabeamformer_amd import host

    _lib()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    vis = str(tmp_path / "vis.bin")                                          # a readable file of visibilities: 4 antennas, no record
    text = ("HDR_VERSION 1.0\nHDR_SIZE 4096\nINSTRUMENT DSA\nCONTENT visibilities\nDTYPE int64\nENDIAN little\nRECORD_HEADER_BYTES 16\n"
            "NANT 4\nNPOL 2\nNFREQ 2\nFIRST_CHANNEL 0\n").encode()
    open(vis, "wb").write(text.ljust(4096, b"\0"))
    other = str(tmp_path / "other.bin")
    _null_file(host, other, 32, 256)
    shifted = str(tmp_path / "shifted.bin")
    _null_file(host, shifted, 64, 256, first_channel=256)
    gains = str(tmp_path / "gains.bin")
    host.write_gains_file(gains, n_ant=64, n_pol=1, n_freq=256, first_channel=0, records=[(0, 1, np.ones((1, 256, 64, 2)), np.ones((1, 256, 2), np.int32))])
    cases = [(["-y", "2"], "-y"),                                            # -y without -E ... -Z
             (["-E", vis, "-G", "g.bin", "-y", "2"], "-y"),                  # -y with the gain solver alone
             (["-Z", other, "-y", "2"], "-y"),                               # -y when the null is applied
             (["-E", vis, "-Z", "n.bin", "-y", "0"], "-y"), (["-E", vis, "-Z", "n.bin", "-y", "5"], "-y"),
             (["-E", vis, "-Z", "n.bin", "-y", "2:-1"], "-y"), (["-E", vis, "-Z", "n.bin", "-y", "two"], "-y"),
             (["-E", vis, "-Z", "n.bin", "-y", "2:x"], "-y"), (["-E", vis, "-Z", "n.bin", "-y", "2x"], "-y"),
             (["-E", vis], "-Z"),                                            # -E without a place for either result
             (["-E", "/nonexistent/vis.bin", "-Z", "n.bin"], "vis.bin"),     # unreadable input
             (["-j", "27", "-E", vis, "-Z", "n.bin"], "-E"),                 # solve mode runs no observation
             (["-Z", "/nonexistent/null.bin"], "null.bin"),                  # unreadable vectors, DEBUG run and observation mode
             (["-j", "27", "-Z", "/nonexistent/null.bin"], "null.bin"),
             (["-Z", other], "NANT"), (["-j", "27", "-Z", other], "NANT"),   # another geometry
             (["-j", "27", "-Z", shifted], "FIRST_CHANNEL"),
             (["-Z", gains], "gains"),                                       # a record file of another kind
             (["-e", "m.bin", "-O", "a.txt", "-Z", other], "-e")]
    for args, word in cases:
        r = subprocess.run([BEAM] + args, capture_output=True, text=True, timeout=60, env=env, cwd=str(tmp_path))
        assert r.returncode != 0 and word in r.stderr and "GPUassert" not in r.stderr and "Selected" not in r.stdout, (args, r.stderr)
    assert not os.path.exists(str(tmp_path / "n.bin")) and not os.path.exists(str(tmp_path / "g.bin"))   # and nothing was created
    # the right geometry passes the checks and stops at the missing device; so do solve mode with valid options and -G ... -Z together
    good = str(tmp_path / "good.bin")
    _null_file(host, good, 64, 256, n_null=2)
    for args in (["-Z", good], ["-A", gains, "-Z", good], ["-E", vis, "-Z", "n.bin", "-y", "4:0"], ["-E", vis, "-G", "g.bin", "-Z", "n.bin", "-y", "1"]):
        r = subprocess.run([BEAM] + args, capture_output=True, text=True, timeout=60, env=env, cwd=str(tmp_path))
        assert r.returncode != 0 and "-Z" not in r.stderr and "-y" not in r.stderr and "GPUassert" in r.stderr, (args, r.stderr)
    # a sharded run reads null_file.<rank>, against the rank's share of the band
    _null_file(host, str(tmp_path / "shard.bin.1"), 64, 128, first_channel=128)
    r = subprocess.run([BEAM, "-j", "27", "-R", "2", "-r", "1", "-I", "id", "-Z", "shard.bin"], capture_output=True, text=True, timeout=60, env=env,
                       cwd=str(tmp_path))
    assert r.returncode != 0 and "-Z" not in r.stderr and "GPUassert" in r.stderr, r.stderr
    r = subprocess.run([BEAM, "-j", "27", "-R", "2", "-r", "0", "-I", "id", "-Z", "shard.bin"], capture_output=True, text=True, timeout=60, env=env,
                       cwd=str(tmp_path))
    assert r.returncode != 0 and "shard.bin.0" in r.stderr and "GPUassert" not in r.stderr, r.stderr
    open(good, "ab").write(b"\0" * 5)                                        # a truncated record
    r = subprocess.run([BEAM, "-Z", good], capture_output=True, text=True, timeout=60, env=env, cwd=str(tmp_path))
    assert r.returncode != 0 and "good.bin" in r.stderr and "GPUassert" not in r.stderr


def test_extended_usage_lists_the_options():
    _lib()
    r = subprocess.run([BEAM, "-H"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and " -E vis_file -Z null_file [-y n_null[:min_ratio]]" in r.stdout and " -Z null_file  " in r.stdout and "spatial null" in r.stdout
    h = subprocess.run([BEAM, "-h"], capture_output=True, text=True, timeout=60)
    assert all(o not in h.stdout for o in ("-Z", "-y "))                     # the reference's own text stays as it is


def test_the_null_file_round_trip(tmp_path):
    from dsabeamformer_amd import host

    rng = np.random.default_rng(9)
    recs = [(7 * i, 4096 + i, rng.standard_normal((3, 2, 8, 2)), rng.standard_normal((3, 3)), rng.integers(0, 200, size=(3, 5)).astype(np.int32))
            for i in range(3)]
    path = str(tmp_path / "null.bin")
    host.write_null_file(path, n_ant=8, n_freq=3, first_channel=128, n_null=2, records=recs)
    assert os.path.getsize(path) == 4096 + 3 * (16 + 3 * 2 * 8 * 16 + 3 * 3 * 8 + 3 * 5 * 4)
    hdr, got = host.read_null_file(path)
    assert hdr["CONTENT"] == "nullvecs" and hdr["DTYPE"] == "float64" and hdr["LAYOUT"] == "freq,vec,ant,reim" and int(hdr["HDR_SIZE"]) == 4096
    assert (int(hdr["NANT"]), int(hdr["NFREQ"]), int(hdr["FIRST_CHANNEL"]), int(hdr["NNULL"])) == (8, 3, 128, 2)
    assert len(got) == 3
    for (b, c, v, e, i), (b2, c2, v2, e2, i2) in zip(recs, got):
        assert (b, c) == (b2, c2) and np.array_equal(_bits(v), _bits(v2)) and np.array_equal(_bits(e), _bits(e2)) and np.array_equal(i, i2)
        assert i2.dtype == np.int32
