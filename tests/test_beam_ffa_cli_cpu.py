"""CPU checks of the `beam` driver's periodicity-search options (csrc/beam_main.cpp, docs/PERIODICITY.md section 5): what the command
line refuses before any device is touched."""
import os
import subprocess

from conftest import ROOT

BEAM = os.path.join(ROOT, "dsabeamformer_amd", "beam")


def _beam(*args):
    from dsabeamformer_amd import build as b

    b.build()
    return subprocess.run([BEAM] + list(args), capture_output=True, text=True, timeout=60)


def test_ffa_without_the_dm_stage_is_refused():
    for args in (("--ffa", "8:13"), ("-j", "8", "--ffa", "64:128", "--ffa-seg", "8192", "--ffa-dec", "4", "--ffa-oct", "3", "--ffa-widths", "5", "--ffa-snr", "9.5",
                                     "--ffa-out", "/dev/null")):
        r = _beam(*args)
        assert r.returncode != 0 and "--ffa (periodicity search) requires the DM stage: give -M dm_max" in r.stderr, r.stderr
        assert "GPUassert" not in r.stderr


def test_ffa_options_without_ffa_and_malformed_ones_are_refused():
    for args in (("--ffa-seg", "64"), ("--ffa-dec", "2"), ("--ffa-oct", "2"), ("--ffa-widths", "2"), ("--ffa-snr", "7"), ("--ffa-out", "x")):
        r = _beam("-M", "40", *args)
        assert r.returncode != 0 and "belong to the periodicity search: give --ffa P_LO:P_HI" in r.stderr, (args, r.stderr)
    for args in (["--ffa", "8"], ["--ffa", "8:"], ["--ffa", ":13"], ["--ffa", "8:13:2"], ["--ffa", "a:b"], ["--ffa", "-8:13"], ["--ffa", "8:13x"],
                 ["--ffa", "8:13", "--ffa-seg", "64k"], ["--ffa", "8:13", "--ffa-dec", "-2"], ["--ffa", "8:13", "--ffa-oct", "1.5"],
                 ["--ffa", "8:13", "--ffa-widths", ""], ["--ffa", "8:13", "--ffa-snr", "high"], ["--ffa", "8:13", "--ffa-snr", "nan"],
                 ["--ffa", "8:13", "--ffa-snr", "7x"]):
        r = _beam("-M", "40", *args)
        assert r.returncode != 0 and "malformed number" in r.stderr and "--ffa P_LO:P_HI" in r.stderr, (args, r.stderr)
        assert "GPUassert" not in r.stderr


def test_extended_usage_lists_the_ffa_options():
    r = _beam("-H")
    assert r.returncode == 0
    for word in ("--ffa P_LO:P_HI", "--ffa-seg N", "--ffa-dec N", "--ffa-oct N", "--ffa-widths K", "--ffa-snr SNR", "--ffa-out FILE"):
        assert word in r.stdout
