"""CPU checks of the `beam` driver's pulsar-folding options (csrc/beam_main.cpp, docs/PULSAR_FOLDING.md section 5): what the command
line refuses before any device is touched."""
import os
import subprocess

from conftest import ROOT

BEAM = os.path.join(ROOT, "dsabeamformer_amd", "beam")


def _beam(*args):
    from dsabeamformer_amd import build as b

    b.build()
    return subprocess.run([BEAM] + list(args), capture_output=True, text=True, timeout=60)


def test_fold_without_the_dm_stage_is_refused():
    for args in (("--fold", "3.3"), ("-j", "8", "--fold", "3.3:-2e-3:0.25", "--fold-dm", "20", "--fold-bins", "16", "--fold-rows", "512", "--fold-out", "/dev/null")):
        r = _beam(*args)
        assert r.returncode != 0 and "--fold (pulsar folding) requires the DM stage: give -M dm_max" in r.stderr, r.stderr
        assert "GPUassert" not in r.stderr


def test_fold_options_without_fold_and_malformed_ones_are_refused():
    for args in (("-M", "40", "--fold-dm", "20"), ("-M", "40", "--fold-bins", "16"), ("-M", "40", "--fold-rows", "64"), ("-M", "40", "--fold-out", "x")):
        r = _beam(*args)
        assert r.returncode != 0 and "belong to the pulsar folder: give --fold" in r.stderr, (args, r.stderr)
    five = sum((["--fold", str(1.0 + k)] for k in range(5)), [])
    for args in (five, ["--fold", "abc"], ["--fold", "3.3:"], ["--fold", "1:2:3:4"], ["--fold", "3.3", "--fold-dm", "-1"], ["--fold", "3.3", "--fold-dm", "1", "--fold-dm", "2"],
                 ["--fold", "3.3", "--fold-bins", "1"], ["--fold", "3.3", "--fold-bins", "4097"], ["--fold", "3.3", "--fold-bins", "16x"],
                 ["--fold", "3.3", "--fold-rows", "-4"]):
        r = _beam("-M", "40", *args)
        assert r.returncode != 0 and "malformed, too many or out of range" in r.stderr, (args, r.stderr)
        assert "GPUassert" not in r.stderr


def test_extended_usage_lists_the_fold_options():
    r = _beam("-H")
    assert r.returncode == 0
    for word in ("--fold F0[:F1[:PHASE0]]", "--fold-dm DM", "--fold-bins N", "--fold-rows ROWS", "--fold-out FILE"):
        assert word in r.stdout
