"""GPU test of the production loop with every stage in ONE run: the order in which the stages follow a launch on its queue, are
delivered and report at the end.  Three `beam -j 33` runs (25 burn-in reads + 8 analysed blocks): A with everything on, B with only
the stages on the DM side, C with only the taps on the voltage blocks.  Whatever A writes must be what B or C writes, and A's closing
lines are theirs, in the loop's order.  Then the lab switch that turns block launches off after the options have passed: the four
stages that need block launches refuse it before anything is launched."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from dm_side import closing_lines, sorted_records  # noqa: E402  (shared with tests/test_gpu_trial_split.py)

pytestmark = pytest.mark.gpu

COMMON = ["-j", "33", "-i", "255"]   # (the incoherent beam is a column of the detected stream: in all three)
# the option values of each stage's own end-to-end test (test_gpu_stamps, _vcut, _cond, _psr, _ffa, _inj, _corr, _sk, _stokes)
DM_SIDE = ["-M", "250", "-N", "8", "-S", "4", "-B", "6", "-n", "4", "-W", "dm.bin", "-C", "cands.txt", "--events", "ev.txt", "--stamps", "st.bin",
           "--voltages", "v.bin", "--voltage-units", "2",
           "--fold", "31.7:-0.4:0.3", "--fold-dm", "25", "--fold", "1200", "--fold-bins", "16", "--fold-rows", "512", "--fold-out", "folds.bin",
           "--ffa", "8:13", "--ffa-seg", "64", "--ffa-dec", "2", "--ffa-oct", "2", "--ffa-widths", "2", "--ffa-snr", "3.0", "--ffa-out", "ffa.txt",
           "--inject", "356:100:3:2e5:1:8", "--inject-train", "400:50:5:3e4", "--inject-out", "truth.txt"]
DM_FILES = ("dm.bin", "cands.txt", "ev.txt", "folds.bin", "ffa.txt", "truth.txt")   # + st.bin and v.bin, compared as sorted records
VOLTAGE_SIDE = ["-V", "vis.bin", "-L", "2", "-Y", "sk.bin", "-J", "2", "-x", "stokes.bin", "-b", "0,100,255", "-w", "det.bin"]
VOLTAGE_FILES = ("vis.bin", "sk.bin", "stokes.bin", "det.bin")

# the closing lines of run_observation, in its order; and which run has the same line
CLOSING = [("DM stage:", "b"), ("Conditioner:", "b"), ("Incoherent beam:", "b"), ("Correlator:", "c"), ("Voltage moments:", "c"), ("Stokes beams:", "c"),
           ("Injector:", "b"), ("Pulsar folder:", "b"), ("Periodicity search:", "b"), ("Single-pulse search:", "b"), ("Events:", "b"), ("Voltage cuts:", "b")]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from dsabeamformer_amd import build

    out = {}
    for name, args in (("a", DM_SIDE + VOLTAGE_SIDE), ("b", DM_SIDE), ("c", VOLTAGE_SIDE)):
        cwd = tmp_path_factory.mktemp(name)
        r = subprocess.run([build.BEAM] + COMMON + args, capture_output=True, text=True, timeout=300, cwd=cwd)
        assert r.returncode == 0, (name, r.stdout[-3000:] + r.stderr)
        out[name] = (str(cwd), r.stdout)
    return out


def test_every_file_of_the_full_run_is_the_file_of_a_partial_run(runs):
    from dsabeamformer_amd import host

    for other, names in (("b", DM_FILES), ("c", VOLTAGE_FILES)):
        for n in names:
            got, want = open(os.path.join(runs["a"][0], n), "rb").read(), open(os.path.join(runs[other][0], n), "rb").read()
            assert got == want and (len(got) > 4096 or not n.endswith(".bin")), n   # (a binary file: more than its header)
    # the cuts: a retried one lands a deliver later, and when a deliver comes depends on the clock -- the same records in any order
    for n, read, key in (("st.bin", host.read_stamp_file, ("t0", "dm", "beam", "tbin", "width", "snr")), ("v.bin", host.read_voltage_file, ("t0", "dm", "beam", "width", "snr"))):
        records = {run: sorted_records(os.path.join(runs[run][0], n), read, key) for run in ("a", "b")}
        assert len(records["a"][1]) >= 1, n
        assert records["a"] == records["b"], n
    for n in ("cands.txt", "ev.txt", "ffa.txt"):   # the run is one at which the search stages find something
        assert np.loadtxt(os.path.join(runs["a"][0], n), ndmin=2).shape[0] >= 1, n


def test_closing_lines_in_the_loops_order_each_as_in_the_partial_run(runs):
    got = closing_lines(runs["a"][1])
    assert [l.split(":")[0] + ":" for l in got] == [title for title, _ in CLOSING], got
    for line, (title, other) in zip(got, CLOSING):
        assert line in closing_lines(runs[other][1]), (line, closing_lines(runs[other][1]))


@pytest.mark.parametrize("args,message", [
    (["-M", "250"], "run_observation: the DM stage needs block-granular launches"),
    (["-V", "vis.bin"], "run_observation: the correlator needs block-granular launches"),
    (["-Y", "sk.bin"], "run_observation: the voltage moments need block-granular launches"),
    (["-x", "stokes.bin", "-b", "0,100,255"], "run_observation: the Stokes beams need block-granular launches"),
], ids=["dm", "correlator", "moments", "stokes"])
def test_unit_launches_are_refused_by_the_stages_that_need_block_launches(tmp_path, args, message):
    """DSABF_UNIT_LAUNCH=1 (a lab switch) turns block launches off behind the options' own check: the plan refuses, after the handle
    exists and before anything is launched."""
    from dsabeamformer_amd import build

    r = subprocess.run([build.BEAM, "-j", "27"] + args, capture_output=True, text=True, timeout=300, cwd=tmp_path,
                       env=dict(os.environ, DSABF_LAB="1", DSABF_UNIT_LAUNCH="1"))
    assert r.returncode != 0 and message in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr)
    assert "obs Complete" not in r.stdout and "Synchronized" not in r.stdout
