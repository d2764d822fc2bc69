"""CPU checks of the `beam` driver's --ffa-detrend option (csrc/beam_main.cpp, docs/PERIODICITY.md section 5): what the command line
refuses before any device is touched, and the extended usage."""
import os
import subprocess

from conftest import ROOT

BEAM = os.path.join(ROOT, "dsabeamformer_amd", "beam")


def _beam(*args):
    from dsabeamformer_amd import build as b

    b.build()
    return subprocess.run([BEAM] + list(args), capture_output=True, text=True, timeout=60)


def test_ffa_detrend_without_ffa_is_refused():
    for args in (("-M", "40", "--ffa-detrend", "8:5"), ("--ffa-detrend", "8:5")):
        r = _beam(*args)
        assert r.returncode != 0 and "belong to the periodicity search: give --ffa P_LO:P_HI" in r.stderr and "--ffa-detrend" in r.stderr, (args, r.stderr)
        assert "GPUassert" not in r.stderr


def test_malformed_ffa_detrend_is_refused():
    for value in ("8", "8:", ":5", "8:5:1", "a:b", "-8:5", "8:5x", "8.5:5", "8:-5", ""):
        r = _beam("-M", "40", "--ffa", "8:13", "--ffa-detrend", value)
        assert r.returncode != 0 and "malformed number" in r.stderr and "--ffa P_LO:P_HI" in r.stderr and "--ffa-detrend BLK:WIN" in r.stderr, (value, r.stderr)
        assert "GPUassert" not in r.stderr
    # ... and without the DM stage the first refusal is still the DM stage's
    r = _beam("--ffa", "8:13", "--ffa-detrend", "8:5")
    assert r.returncode != 0 and "--ffa (periodicity search) requires the DM stage: give -M dm_max" in r.stderr


def test_extended_usage_lists_ffa_detrend():
    r = _beam("-H")
    assert r.returncode == 0 and "--ffa-detrend BLK:WIN" in r.stdout and "detrend=BLK:WIN" in r.stdout
