"""CPU checks of the correlator (docs/CORRELATOR.md): the numpy oracle against a per-byte Python loop, the known answer, the
Hermitian square, the exports' error convention without a handle or stage, bf_corr_entries and the `beam -V / -L` command line.
No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import corr_oracle  # noqa: E402

BEAM = os.path.join(ROOT, "dsabeamformer_amd", "beam")
BF_ERR_INVALID = -1


def _lib():
    from dsabeamformer_amd import _lib as l
    from dsabeamformer_amd import build as b

    b.build()
    return l.load()


def _nibbles(b):
    re, im = b >> 4, b & 15
    return (re - 16 if re & 8 else re), (im - 16 if im & 8 else im)


def test_oracle_equals_a_per_byte_loop_on_every_code():
    assert [(int(r), int(m)) for r, m in zip(corr_oracle.RE, corr_oracle.IM)] == [_nibbles(b) for b in range(256)]
    # every code once, in a layout with more than one unit, channel, column and polarisation: [2][2][8 * 2][4]
    rng = np.random.default_rng(7)
    n_u, n_f, n_c, n_pol, n_a = 2, 2, 8, 2, 4
    packed = rng.permutation(256).astype(np.uint8).reshape(n_u, n_f, n_c * n_pol, n_a)
    got = corr_oracle.visibilities(packed, n_pol)
    assert got.shape == (n_f, n_pol, 10, 2) and got.dtype == np.int64
    for f in range(n_f):
        for p in range(n_pol):
            for a1 in range(n_a):
                for a2 in range(a1 + 1):
                    acc = 0
                    for u in range(n_u):
                        for c in range(n_c):
                            r1, m1 = _nibbles(int(packed[u, f, c * n_pol + p, a1]))
                            r2, m2 = _nibbles(int(packed[u, f, c * n_pol + p, a2]))
                            acc += complex(r1, m1) * complex(r2, -m2)
                    assert tuple(got[f, p, corr_oracle.bl(a1, a2)]) == (int(acc.real), int(acc.imag)), (f, p, a1, a2)
    assert np.all(got[:, :, [corr_oracle.bl(a, a) for a in range(n_a)], 1] == 0)          # the diagonal: autocorrelations
    assert np.array_equal(corr_oracle.visibilities_f64(packed, n_pol), got)                # the float64 route: the same bits
    big = rng.integers(0, 256, size=(3, 2, 66, 20), dtype=np.uint8)
    assert np.array_equal(corr_oracle.visibilities_f64(big, 2), corr_oracle.visibilities(big, 2))
    assert np.array_equal(corr_oracle.visibilities_f64(big, 1), corr_oracle.visibilities(big, 1))
    assert [corr_oracle.bl(0, 0), corr_oracle.bl(1, 0), corr_oracle.bl(1, 1), corr_oracle.bl(2, 0), corr_oracle.bl(255, 255)] == [0, 1, 2, 3, 32895]
    assert corr_oracle.supported(256, 2 ** 24 - 1) and not corr_oracle.supported(256, 2 ** 24) and not corr_oracle.supported(260, 1)


def test_the_known_answer_pins_the_conjugated_operand_and_the_row():
    packed = np.frombuffer(corr_oracle.KNOWN_BYTES, np.uint8).reshape(1, 1, 1, 4)
    v = corr_oracle.visibilities(packed, 1)[0, 0]
    for (a1, a2), want in corr_oracle.KNOWN.items():
        assert tuple(v[corr_oracle.bl(a1, a2)]) == want
    assert tuple(v[corr_oracle.bl(1, 0)]) == (29, 29) and tuple(v[corr_oracle.bl(1, 1)]) == (58, 0) and tuple(v[corr_oracle.bl(0, 0)]) == (29, 0)
    assert not v[corr_oracle.bl(2, 0):].any()


def test_to_square_is_hermitian_in_both_implementations():
    from dsabeamformer_amd import api

    rng = np.random.default_rng(11)
    packed = rng.integers(0, 256, size=(2, 3, 10, 8), dtype=np.uint8)
    tri = corr_oracle.visibilities(packed, 2)
    for fn in (corr_oracle.to_square, api.vis_to_square):
        sq = fn(tri, 8)
        assert sq.shape == (3, 2, 8, 8) and sq.dtype == np.complex128
        assert np.array_equal(sq, np.conj(np.swapaxes(sq, -1, -2)))
        assert np.all(np.diagonal(sq, axis1=-2, axis2=-1).imag == 0)
        assert sq[1, 1, 5, 2] == complex(*tri[1, 1, corr_oracle.bl(5, 2)]) and sq[1, 1, 2, 5] == complex(*tri[1, 1, corr_oracle.bl(5, 2)]).conjugate()
    # against the definition, as a complex outer product
    v = (corr_oracle.RE[packed] + 1j * corr_oracle.IM[packed]).reshape(2, 3, 5, 2, 8)
    assert np.array_equal(corr_oracle.to_square(tri, 8), np.einsum("ufcpa,ufcpb->fpab", v, np.conj(v)))


def test_every_new_export_refuses_a_null_handle_or_stage():
    lib = _lib()
    out, n = C.c_void_p(), C.c_uint64()
    calls = [lambda: lib.bf_correlate_device(None, None, 1, None, 0, None),
             lambda: lib.bf_corr_create(None, 2, C.byref(out)),
             lambda: lib.bf_corr_create(None, 2, None),
             lambda: lib.bf_corr_push(None, None, 1, None),
             lambda: lib.bf_corr_push_block(None, 0, 0, 0, 1),
             lambda: lib.bf_corr_dump(None, None),
             lambda: lib.bf_corr_collect(None, None, C.byref(n)),
             lambda: lib.bf_corr_pending(None)]
    for i, call in enumerate(calls):
        assert call() == BF_ERR_INVALID and lib.bf_last_error(), i
    assert out.value is None
    assert lib.bf_corr_destroy(None) == 0                                   # like free(): nothing to destroy


def test_corr_entries_at_c3_and_at_four_antennas():
    from dsabeamformer_amd import api

    lib = _lib()
    c3 = api.production_config()
    assert (c3.n_ant, c3.n_pol, c3.n_freq) == (64, 2, 256)
    assert lib.bf_corr_entries(C.byref(c3)) == 256 * 2 * 2080
    assert lib.bf_corr_entries(C.byref(api.debug_config(n_ant=4, n_freq=3, n_pol=1))) == 3 * 10
    assert lib.bf_corr_entries(None) == 0


def test_beam_usage_errors_come_before_any_device():
    _lib()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")     # no device either way: the refusal must not need one
    cases = [(["-V", "vis.bin"], "-V"),                                     # the correlator without the observation mode
             (["-j", "27", "-V", "vis.bin", "-L", "0"], "-L"),              # -L < 1
             (["-j", "27", "-V", "vis.bin", "-L", "-3"], "-L"),
             (["-j", "27", "-L", "2"], "-L"),                               # -L without -V
             (["-L", "2"], "-L")]
    for args, opt in cases:
        r = subprocess.run([BEAM] + args, capture_output=True, text=True, timeout=60, env=env, cwd=os.path.join(ROOT, "tests"))
        assert r.returncode != 0 and opt in r.stderr and "GPUassert" not in r.stderr and "Selected" not in r.stdout, (args, r.stderr)
    assert not os.path.exists(os.path.join(ROOT, "tests", "vis.bin"))       # and nothing was created


def test_extended_usage_lists_the_options():
    _lib()
    r = subprocess.run([BEAM, "-H"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and " -V file " in r.stdout and "-L corr_blocks" in r.stdout and "correlator" in r.stdout
    h = subprocess.run([BEAM, "-h"], capture_output=True, text=True, timeout=60)
    assert "-V" not in h.stdout and "-L" not in h.stdout                    # the reference's own text stays as it is


def test_python_surface_and_signature_table():
    from dsabeamformer_amd import _lib as l
    from dsabeamformer_amd import api, host

    names = ["bf_correlate_device", "bf_corr_entries", "bf_corr_create", "bf_corr_destroy", "bf_corr_push", "bf_corr_push_block",
             "bf_corr_dump", "bf_corr_collect", "bf_corr_pending"]
    assert all(n in l.SIGNATURES for n in names)
    assert l.SIGNATURES["bf_corr_entries"][0] is C.c_size_t and l.SIGNATURES["bf_corr_push_block"][1] == [C.c_void_p] + [C.c_int] * 4
    assert callable(api.Beamformer.correlate) and callable(api.vis_to_square) and callable(host.read_vis_file)
    assert all(callable(getattr(api.Correlator, m)) for m in ("push", "push_block", "dump", "collect", "close"))
    assert isinstance(api.Correlator.pending, property)


def test_vis_file_round_trip(tmp_path):
    """A file in dsabf::vis_file_sink's layout (include/dsabf_host.hpp), written here with numpy: the 4096-byte `KEY value` header, NUL
    padded, then per dump two uint64 and the int64 entries.  host.read_vis_file returns exactly the header and the records."""
    from dsabeamformer_amd import host

    n_ant, n_pol, n_freq = 5, 2, 3
    shape = (n_freq, n_pol, n_ant * (n_ant + 1) // 2, 2)
    rng = np.random.default_rng(31)
    records = [(0, 4096, rng.integers(-2**62, 2**62, shape, dtype=np.int64)), (6, 1, rng.integers(-2**62, 2**62, shape, dtype=np.int64))]
    text = ("HDR_VERSION 1.0\nHDR_SIZE 4096\nINSTRUMENT DSA\nCONTENT visibilities\nDTYPE int64\nENDIAN little\n"
            "LAYOUT freq,pol,baseline(lower triangle a1*(a1+1)/2+a2),reim\nRECORD_HEADER_BYTES 16\nNANT %d\nNPOL %d\nNFREQ %d\n"
            "FIRST_CHANNEL 128\nN_OUTPUTS_PER_GEMM 2\nN_GEMMS_PER_BLOCK 4\nN_AVERAGING 16\nGPU 1\n" % (n_ant, n_pol, n_freq)).encode()
    path = str(tmp_path / "v.bin")
    with open(path, "wb") as fp:
        fp.write(text.ljust(4096, b"\0"))
        for first_block, n_columns, vis in records:
            fp.write(np.array([first_block, n_columns], "<u8").tobytes() + vis.astype("<i8").tobytes())
    hdr, dumps = host.read_vis_file(path)
    assert hdr["CONTENT"] == "visibilities" and hdr["DTYPE"] == "int64" and hdr["LAYOUT"] == "freq,pol,baseline(lower triangle a1*(a1+1)/2+a2),reim"
    assert (int(hdr["NANT"]), int(hdr["NPOL"]), int(hdr["NFREQ"]), int(hdr["FIRST_CHANNEL"]), int(hdr["HDR_SIZE"]), int(hdr["GPU"])) == (5, 2, 3, 128, 4096, 1)
    assert [(d[0], d[1]) for d in dumps] == [(0, 4096), (6, 1)]
    assert all(d[2].dtype == np.int64 and d[2].shape == shape and np.array_equal(d[2], r[2]) for d, r in zip(dumps, records))
    assert os.path.getsize(path) == 4096 + 2 * (16 + records[0][2].nbytes)
