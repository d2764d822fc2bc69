"""CPU checks of the `beam` driver's pulse-injection options (csrc/beam_main.cpp, docs/INJECTION.md section 4): what the command line
refuses before any device is touched."""
import os
import subprocess

from conftest import ROOT

BEAM = os.path.join(ROOT, "dsabeamformer_amd", "beam")


def _beam(*args):
    from dsabeamformer_amd import build as b

    b.build()
    return subprocess.run([BEAM] + list(args), capture_output=True, text=True, timeout=60)


def test_injection_without_the_dm_stage_is_refused():
    for args in (("--inject", "300:20:3:6"), ("--inject-train", "3.3:20:3:0.5"), ("--inject-out", "/dev/null"),
                 ("-j", "8", "--inject", "300:20:3:6:1.5:16", "--inject-train", "3.3:20:3:0.5:0.1:32", "--inject-out", "/dev/null")):
        r = _beam(*args)
        assert r.returncode != 0 and "(pulse injection) require the DM stage: give -M dm_max" in r.stderr, (args, r.stderr)
        assert "GPUassert" not in r.stderr


def test_inject_out_without_a_pulse_is_refused():
    r = _beam("-M", "40", "--inject-out", "x")
    assert r.returncode != 0 and "--inject-out belongs to the pulse injection: give --inject" in r.stderr, r.stderr
    assert "GPUassert" not in r.stderr and not os.path.exists("x")


def test_too_many_trains_and_malformed_numbers_are_refused():
    five = sum((["--inject-train", "%g:20:3:0.5" % (1.0 + k)] for k in range(5)), [])
    for args in (five,
                 ["--inject", "abc"], ["--inject", "300:20:3"], ["--inject", "300:20:3:6:"], ["--inject", "300:20:3:6:1:8:9"], ["--inject", "300:20:3:6x"],
                 ["--inject", "-1:20:3:6"], ["--inject", "300.5:20:3:6"], ["--inject", "300:-2:3:6"], ["--inject", "300:20:-1:6"], ["--inject", "300:20:2.5:6"],
                 ["--inject", "300:20:3:nan"], ["--inject", "300:20:3:6:0"], ["--inject", "300:20:3:6:-1"], ["--inject", "300:20:3:6:1:0"],
                 ["--inject", "300:20:3:6:1:4097"], ["--inject", "300:20:3:6:1:7.5"], ["--inject", "300:20:3:6:1000"],
                 ["--inject-train", "3.3:20:3"], ["--inject-train", "3.3:-1:3:0.5"], ["--inject-train", "3.3:20:3:0.5:0"], ["--inject-train", "3.3:20:3:0.5:1.5"],
                 ["--inject-train", "3.3:20:3:0.5:0.1:1"], ["--inject-train", "3.3:20:3:0.5:0.1:4097"], ["--inject-train", "inf:20:3:0.5"]):
        r = _beam("-M", "40", *args)
        assert r.returncode != 0 and "malformed, too many or out of range" in r.stderr, (args, r.stderr)
        assert "GPUassert" not in r.stderr


def test_extended_usage_lists_the_injection_options():
    r = _beam("-H")
    assert r.returncode == 0
    for word in ("--inject T0:DM:BEAM:FLUENCE[:SIGMA[:W]]", "--inject-train F0:DM:BEAM:AMP[:DUTY[:BINS]]", "--inject-out FILE"):
        assert word in r.stdout
