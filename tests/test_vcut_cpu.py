"""CPU-side checks of the voltage history (include/dsabf.h: bf_vhist_*; docs/VOLTAGE_CUTS.md): the oracle against a per-byte loop, the sizing
helper against the derivation worked by hand, every new export on a NULL stage or handle, the ctypes table and the api surface, the
`beam` command line's usage errors, and the voltage file through the header's sink, the C wrappers and host.read_voltage_file.  No GPU."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import vcut_oracle as vo  # noqa: E402

BF_ERR_INVALID, BF_ERR_STATE = -1, -4


@pytest.fixture(scope="module")
def api():
    from dsabeamformer_amd import api as a
    from dsabeamformer_amd import build

    build.build()
    return a


def test_the_oracle_against_a_per_byte_loop_with_a_wrap_inside_a_run():
    """Fancy indexing over the whole series against the contract read literally -- physical unit (s / S) mod cap_units, sample s % S -- on
    windows whose runs begin in the ring's last physical unit and end in its first, inside a run (j0 > 0) and on its boundary."""
    rng = np.random.default_rng(3)
    n_f, S, B, cap = 3, 4, 8, 5
    units = rng.integers(0, 256, size=(12, n_f, S, B), dtype=np.uint8)           # units 7 .. 11 are in the ring: physical 2, 3, 4, 0, 1
    delays = np.array([[0, 0, 0], [0, 3, 9], [1, S, S + 1]], np.int32)
    wrapped = 0
    for dm in range(3):
        for n_out in (1, 2):
            sp = vo.span(delays, dm, n_out, S)
            for t0 in range(7 * S, 12 * S - sp + 1):
                assert vo.status(delays, t0, dm, n_out, S, 7, 12) == 0
                a = vo.window(units, delays, t0, dm, n_out)
                assert np.array_equal(a, vo.window_by_loop(units, delays, t0, dm, n_out, cap)), (dm, n_out, t0)
                s0 = t0 + delays[dm]
                wrapped += int((((s0 // S) % cap == cap - 1) & (s0 % S != 0)).any())
            assert vo.status(delays, 7 * S - 1, dm, n_out, S, 7, 12) == 1 and vo.status(delays, 12 * S - sp + 1, dm, n_out, S, 7, 12) == 2
    assert wrapped >= 10
    out, st = vo.cut(units, delays, [(7 * S, 1), (7 * S - 1, 1), (11 * S, 1), (0, 2)], 1, 7, 12)
    assert list(st) == [0, 1, 2, 1] and out.shape == (4, 1, n_f, S, B)
    assert np.array_equal(out[0], vo.window(units, delays, 7 * S, 1, 1)) and (out[1:] == vo.SENTINEL).all()
    # the status rule where both hold: a window longer than the ring
    assert vo.status(delays, 7 * S - 1, 0, 6, S, 7, 12) == 1 and vo.status(delays, 7 * S, 0, 6, S, 7, 12) == 2


def test_units_needed_is_the_derivation_worked_by_hand(api):
    """The geometry of tools/stamp_time.py: C3 (16 rows per unit, 32 units per block), pushes of 512 rows, largest delay 123 rows, three chunks
    in flight, t_tol 0, widths up to 32, cuts of 2 units.  Rows (docs/VOLTAGE_CUTS.md section 3):
      the DM stage's own        123 + 3 * 512                     = 1659
      half a cut                2 * 16 / 2                        =   16
      t_tol + max_width         0 + 32                            =   32
      pushes in flight          (3 + 1) * 512                     = 2048      -> 3755 rows = 234.7 units -> 235, + 1 (a window may begin
      inside a unit) + 32 (a block of units in flight)                        = 268 units."""
    import dsabeamformer_amd as bfm

    c3 = bfm.production_config(n_out_per_gemm=16)
    assert (c3.n_out_per_gemm, c3.n_gemms_per_block) == (16, 32)
    assert api.vhist_units_needed(c3, 123, 512, 3, 0, 32, 2) == 268
    assert api.vhist_units_needed(c3, 123, 512, 3, 0, 32, 3) == 269              # half a cut is 24 rows: 3763 rows = 235.2 units -> 236
    lib = bfm.load()
    need = lambda *a: lib.bf_vhist_units_needed(C.byref(c3), *a)                 # noqa: E731
    # every term moves the result as the formula says
    assert need(123 + 16, 512, 3, 0, 32, 2) == 269 and need(123, 512, 4, 0, 32, 2) == 268 + 32 and need(123, 512, 3, 16, 32, 2) == 269
    assert need(123, 512, 3, 0, 32 + 16, 2) == 269 and need(123, 512, 3, 0, 32, 4) == 269 and need(0, 16, 0, 0, 0, 1) == (4 * 16 + 8 + 15) // 16 + 1 + 32
    dbg = bfm.debug_config()                                                    # 8 rows per unit
    assert lib.bf_vhist_units_needed(C.byref(dbg), 0, 8, 0, 0, 1, 2) == (3 * 8 + 8 + 1 + 8 + 7) // 8 + 1 + 32
    # undefined: 0
    for bad in ((-1, 512, 3, 0, 32, 2), (123, 0, 3, 0, 32, 2), (123, 512, -1, 0, 32, 2), (123, 512, 3, -1, 32, 2), (123, 512, 3, 0, -1, 2),
                (123, 512, 3, 0, 32, 0)):
        assert need(*bad) == 0, bad
    assert lib.bf_vhist_units_needed(None, 123, 512, 3, 0, 32, 2) == 0


def test_every_new_export_on_a_null_stage_or_handle(api):
    from dsabeamformer_amd import _lib

    lib = _lib.load()
    u, v = C.c_uint64(), C.c_void_p()
    st = (C.c_int32 * 1)(-7)
    req = _lib.BfVcutRequest(0, 0, 0)
    delays = (C.c_int32 * 4)()
    assert lib.bf_vhist_create(None, delays, 1, 1, C.byref(v)) == BF_ERR_INVALID and not v.value and b"handle" in lib.bf_last_error()
    assert lib.bf_vhist_create(None, delays, 1, 1, None) == BF_ERR_INVALID
    assert lib.bf_vhist_push(None, delays, 1, None) == BF_ERR_INVALID
    assert lib.bf_vhist_push_block(None, 0, 0, 0, 1) == BF_ERR_INVALID
    assert lib.bf_vhist_history(None, C.byref(u), C.byref(u), C.byref(u)) == BF_ERR_INVALID
    assert lib.bf_vhist_cut(None, C.byref(req), 1, 1, delays, st, None) == BF_ERR_INVALID
    assert lib.bf_vhist_cut_host(None, C.byref(req), 1, 1, delays, st) == BF_ERR_INVALID
    assert lib.bf_vhist_destroy(None) == 0 and st[0] == -7
    t = C.c_void_p()
    assert lib.bfh_voltage_sink_deliver(None, 0, 0, 0, 1, 1.0, delays, 16) == BF_ERR_INVALID and lib.bfh_voltage_sink_destroy(None) == 0
    assert lib.bfh_voltage_sink_create(None, None, 1, 0, C.byref(t)) == BF_ERR_INVALID and not t.value


def test_the_lib_table_and_the_api_surface(api):
    from dsabeamformer_amd import _lib

    names = ["bf_vhist_units_needed", "bf_vhist_create", "bf_vhist_destroy", "bf_vhist_push", "bf_vhist_push_block", "bf_vhist_history", "bf_vhist_cut",
             "bf_vhist_cut_host"]
    lib = _lib.load()
    for n in names + ["bfh_voltage_sink_create", "bfh_voltage_sink_deliver", "bfh_voltage_sink_destroy"]:
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES["bf_vhist_cut"][1]) == 7 and len(_lib.SIGNATURES["bf_vhist_cut_host"][1]) == 6
    assert C.sizeof(_lib.BfVcutRequest) == 16 == api.vcut_request_dtype().itemsize and api.vcut_request_dtype().names == ("t0", "dm", "pad")
    for m in ("push", "push_block", "history", "cut", "cut_host", "close"):
        assert hasattr(api.VoltageHistory, m), m
    assert list(inspect.signature(api.VoltageHistory.__init__).parameters)[1:] == ["bf", "delays", "history_units"]
    assert list(inspect.signature(api.VoltageHistory.cut).parameters)[1:] == ["requests", "n_units_out", "d_out", "stream"]
    assert inspect.signature(api.VoltageHistory.cut).parameters["stream"].default == 0
    header = open(os.path.join(ROOT, "include", "dsabf.h")).read()
    for n in names:
        assert n + "(" in header, n
    assert "src/beamformer.hh:124" in header and "src/beamformer.cu:425-431" in header
    # the device code lives in a directory of its own, outside the kernel build id
    from dsabeamformer_amd import build

    assert any(p.endswith(os.path.join("vcut", "bf_vcut.hip")) for p in build.sources())
    assert os.path.exists(os.path.join(build.CSRC, "vcut", "bf_vcut_kernels.h")) and not os.path.exists(os.path.join(build.CSRC, "bf_vcut.hip"))


# ---- the layers above: the `beam` command line and the file ----------------------------------------------------------------------
SEARCH = ["-M", "250", "-S", "6"]
USAGE_ERRORS = [
    (SEARCH + ["--voltages", "v.bin"], "give --events FILE"),                                                   # --voltages without --events
    (["--voltages", "v.bin"], "give --events FILE"),
    (SEARCH + ["--events", "ev.txt", "--voltage-units", "2"], "give --voltages FILE"),                          # the children without the parent
    (SEARCH + ["--events", "ev.txt", "--voltage-history", "64"], "give --voltages FILE"),
    (SEARCH + ["--events", "ev.txt", "--voltage-flagged"], "give --voltages FILE"),
    (SEARCH + ["--events", "ev.txt", "--voltages", "v.bin", "--voltage-units", "0"], "whole number >= 1"),      # numbers < 1, or no numbers
    (SEARCH + ["--events", "ev.txt", "--voltages", "v.bin", "--voltage-units", "-2"], "whole number >= 1"),
    (SEARCH + ["--events", "ev.txt", "--voltages", "v.bin", "--voltage-units", "2x"], "whole number >= 1"),
    (SEARCH + ["--events", "ev.txt", "--voltages", "v.bin", "--voltage-history", "0"], "whole number >= 1"),
    (SEARCH + ["--events", "ev.txt", "--voltages", "v.bin", "--voltage-history", "x"], "whole number >= 1"),
    (SEARCH + ["--events", "ev.txt", "--voltages", "v.bin", "-R", "2", "-r", "0"], "not available in a sharded run"),   # -R
]


@pytest.mark.parametrize("args,message", USAGE_ERRORS, ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_every_usage_error_comes_before_a_device_is_touched(api, tmp_path, args, message):
    from dsabeamformer_amd import build

    r = subprocess.run([build.BEAM, "-j", "27"] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert r.returncode == 1 and message in r.stderr, (r.returncode, r.stderr)
    assert "GPUassert" not in r.stderr and not os.listdir(tmp_path)            # no device was asked for, no file was created


def test_beam_H_lists_the_options_and_h_stays_the_references_text(api):
    from dsabeamformer_amd import build

    big = subprocess.run([build.BEAM, "-H"], capture_output=True, text=True, timeout=60)
    small = subprocess.run([build.BEAM, "-h"], capture_output=True, text=True, timeout=60)
    assert big.returncode == 0 and small.returncode == 0
    for name in ("--voltages FILE", "--voltage-units N", "--voltage-history UNITS", "--voltage-flagged"):
        assert name in big.stdout and name not in small.stdout, name
    assert big.stdout.startswith(small.stdout) and "--" not in small.stdout.replace("---", "")


WRITER = r"""
#include "dsabf_host.hpp"
int main(int argc, char** argv)
{
    bf_config cfg = {};
    cfg.n_ant = 4; cfg.n_freq = 3; cfg.n_pol = 2; cfg.n_avg = 2; cfg.n_out_per_gemm = 5;   // 3 * 10 * 8 = 240 bytes per unit
    dsabf::voltage_file_sink vs(argv[1], cfg, 2, 128);
    if (!vs.is_open()) return 2;
    unsigned char data[2][480];
    for (int k = 0; k < 480; k++) { data[0][k] = (unsigned char)(k * 7 + 1); data[1][k] = (unsigned char)(255 - k); }
    if (!vs.deliver(123456789012345ull, 7, 255, 32, 12.345678901234567, data[0], 480) || !vs.deliver(0, 0, 0, 1, 8.0, data[1], 480)) return 4;
    if (vs.deliver(0, 0, 0, 1, 8.0, data[1], 240)) return 5;   // another size than the header's: refused
    return vs.get_cuts_written() == 2 ? 0 : 6;
}
"""


def _check_file(host, path):
    hdr, cuts = host.read_voltage_file(path)
    assert (hdr["CONTENT"], hdr["DTYPE"], hdr["LAYOUT"]) == ("voltages", "packed4+4", "unit,freq,time,pol,ant")
    assert [hdr[k] for k in ("NANT", "NFREQ", "NPOL", "NAVG", "NOUT", "UNITS", "FIRST_CHANNEL")] == ["4", "3", "2", "2", "5", "2", "128"]
    assert os.path.getsize(path) == 4096 + 2 * (28 + 480) and len(cuts) == 2
    c = cuts[0]
    assert (c["t0"], c["dm"], c["beam"], c["width"], c["snr"]) == (123456789012345, 7, 255, 32, 12.345678901234567)
    k = np.arange(480)
    assert c["data"].shape == (2, 3, 10, 8) and np.array_equal(c["data"].reshape(-1), ((k * 7 + 1) % 256).astype(np.uint8))
    assert (cuts[1]["t0"], cuts[1]["dm"], cuts[1]["beam"], cuts[1]["width"], cuts[1]["snr"]) == (0, 0, 0, 1, 8.0)
    assert np.array_equal(cuts[1]["data"].reshape(-1), ((255 - k) % 256).astype(np.uint8))


def test_the_file_round_trip(api, tmp_path):
    """voltage_file_sink (header-only, like stamp_file_sink) written by a small C++ program, read by host.read_voltage_file; the oracle's
    writer gives the same bytes."""
    from dsabeamformer_amd import host

    src, exe = tmp_path / "writer.cpp", tmp_path / "writer"
    src.write_text(WRITER)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    path = str(tmp_path / "v.bin")
    assert subprocess.run([str(exe), path]).returncode == 0
    _check_file(host, path)
    k = np.arange(480)
    vo.write_file(str(tmp_path / "o.bin"), 4, 3, 2, 2, 5, 2, 128,
                  [(123456789012345, 7, 255, 32, 12.345678901234567, ((k * 7 + 1) % 256).astype(np.uint8)), (0, 0, 0, 1, 8.0, ((255 - k) % 256).astype(np.uint8))])
    assert open(tmp_path / "o.bin", "rb").read() == open(path, "rb").read()


def test_the_file_round_trip_through_the_c_wrappers(api, tmp_path):
    """bfh_voltage_sink_* (include/dsabf_host.h) from Python: the same file; an unwritable path, a geometry that is none and a cut of another
    size are refused."""
    import dsabeamformer_amd as bfm
    from dsabeamformer_amd import host

    lib = bfm.load()
    cfg = bfm.debug_config(n_ant=4, n_freq=3, n_pol=2, n_avg=2, n_out_per_gemm=5)
    path = str(tmp_path / "v.bin")
    t = C.c_void_p()
    for bad in ((None, C.byref(cfg), 2, 128), (path.encode(), None, 2, 128), (path.encode(), C.byref(cfg), 0, 128), (path.encode(), C.byref(cfg), 2, -1),
                (str(tmp_path / "no" / "v.bin").encode(), C.byref(cfg), 2, 128)):
        assert lib.bfh_voltage_sink_create(*bad, C.byref(t)) == BF_ERR_INVALID and not t.value, bad
    assert lib.bfh_voltage_sink_create(path.encode(), C.byref(cfg), 2, 128, None) == BF_ERR_INVALID
    assert lib.bfh_voltage_sink_create(path.encode(), C.byref(cfg), 2, 128, C.byref(t)) == 0
    k = np.arange(480)
    data = [((k * 7 + 1) % 256).astype(np.uint8), ((255 - k) % 256).astype(np.uint8)]
    assert lib.bfh_voltage_sink_deliver(t, 123456789012345, 7, 255, 32, 12.345678901234567, data[0].ctypes.data, 480) == 0
    assert lib.bfh_voltage_sink_deliver(t, 0, 0, 0, 1, 8.0, data[1].ctypes.data, 240) == BF_ERR_STATE            # not the header's size
    assert lib.bfh_voltage_sink_deliver(t, 0, 0, 0, 1, 8.0, None, 480) == BF_ERR_INVALID
    assert lib.bfh_voltage_sink_deliver(t, 0, 0, 0, 1, 8.0, data[1].ctypes.data, 480) == 0
    assert lib.bfh_voltage_sink_destroy(t) == 0
    _check_file(host, path)
