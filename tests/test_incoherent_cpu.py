"""CPU checks of the incoherent beam (docs/INCOHERENT_BEAM.md): the numpy oracle against a per-byte Python loop, the two exports'
error convention without a handle, and the `beam -i` command line.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import ib_oracle  # noqa: E402

BEAM = os.path.join(ROOT, "dsabeamformer_amd", "beam")


def _lib():
    from dsabeamformer_amd import _lib as l
    from dsabeamformer_amd import build as b

    b.build()
    return l.load()


def _byte_power(b):
    re, im = b >> 4, b & 15
    re, im = (re - 16 if re & 8 else re), (im - 16 if im & 8 else im)
    return re * re + im * im


def test_oracle_equals_a_per_byte_loop_on_every_code_and_the_known_answer():
    assert [int(v) for v in ib_oracle.TABLE] == [_byte_power(b) for b in range(256)]
    assert max(ib_oracle.TABLE) == 128 and ib_oracle.TABLE[0x88] == 128
    assert [_byte_power(b) for b in ib_oracle.KNOWN_BYTES] == [58, 29, 100, 49] and ib_oracle.KNOWN_SUM == 236
    known = np.frombuffer(ib_oracle.KNOWN_BYTES, np.uint8).reshape(1, 1, 1, 4)
    assert ib_oracle.incoherent(known, 1, 1).tolist() == [[[236.0]]]
    # every code once, in a layout with more than one unit, channel, output and sample per output: [2][2][2 * 2][16]
    rng = np.random.default_rng(5)
    packed = rng.permutation(256).astype(np.uint8).reshape(2, 2, 4, 16)
    got = ib_oracle.incoherent(packed, n_out=2, n_ipo=2)
    assert got.shape == (2, 2, 2) and got.dtype == np.float32
    for u in range(2):
        for o in range(2):
            for f in range(2):
                want = sum(_byte_power(int(b)) for b in packed[u, f, 2 * o:2 * o + 2].reshape(-1))
                assert got[u, o, f] == want
    assert got.sum() == sum(_byte_power(b) for b in range(256))
    # the bound the feature is defined for, and the DM-0 restatement
    assert ib_oracle.supported(2048, 64) and not ib_oracle.supported(2048, 66) and not ib_oracle.supported(2052, 64)
    col = np.array([[2.0 ** 24, 1.0, 1.0], [1.0, 1.0, 2.0 ** 24]], np.float32)
    assert ib_oracle.dm0_row(col).tolist() == [2.0 ** 24, 2.0 ** 24 + 2]          # ascending f, one fp32 rounding per add


def test_both_exports_refuse_a_null_handle():
    lib = _lib()
    assert lib.bf_incoherent_device(None, None, 1, None, 1, None) == -1 and lib.bf_last_error()
    assert lib.bf_set_incoherent_beam(None, 0) == -1 and b"NULL" in lib.bf_last_error()
    assert lib.bf_set_incoherent_beam(None, -1) == -1


def test_beam_i_outside_the_beams_is_a_usage_error_before_any_device():
    _lib()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")     # no device either way: the refusal must not need one
    for bad in ("256", "-2"):
        for mode in ([], ["-j", "27"]):
            r = subprocess.run([BEAM] + mode + ["-i", bad], capture_output=True, text=True, timeout=60, env=env)
            assert r.returncode != 0 and "-i" in r.stderr and "GPUassert" not in r.stderr and "Selected" not in r.stdout, (bad, mode, r.stderr)
    # a valid index without the observation mode it belongs to: also refused, also naming the option
    r = subprocess.run([BEAM, "-i", "5"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode != 0 and "-i" in r.stderr and "GPUassert" not in r.stderr


def test_extended_usage_lists_the_option():
    _lib()
    r = subprocess.run([BEAM, "-H"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and " -i beam " in r.stdout and "incoherent beam" in r.stdout
    h = subprocess.run([BEAM, "-h"], capture_output=True, text=True, timeout=60)
    assert "-i" not in h.stdout                                                   # the reference's own text stays as it is


def test_python_surface_and_signature_table():
    from dsabeamformer_amd import _lib as l
    from dsabeamformer_amd import api

    assert l.SIGNATURES["bf_incoherent_device"][1][4] is C.c_size_t and l.SIGNATURES["bf_set_incoherent_beam"][1] == [C.c_void_p, C.c_int]
    assert callable(api.Beamformer.incoherent) and callable(api.Beamformer.set_incoherent_beam)
