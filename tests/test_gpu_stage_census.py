"""The census of the stage kernels, GPU side (-m gpu): every kernel instantiation compiled from csrc/<stage>/ is launched once, on the
smallest input that selects it, and held to its stage's oracle to the bit (tests/support/stage_census.py: one row each).  WHICH kernel a
call ran is what the launcher itself recorded (include/dsabf_bench.h: bf_stage_launches) -- for the Stokes beams it depends on the chip's
CU count, so nothing here restates a launcher's switch: a row passes only if the name it claims is among the names recorded while it
ran, and at the end everything recorded is exactly tools/census.py::stage_compiled().

ONE test function that loops over the whole table: nothing is parametrised, so the sweep cap of conftest.py thins nothing.  The
per-kernel report is printed, and written into the directory DSABF_REPORT_DIR names, if it names one (committed as
profiles/stage_census_gpu.txt)."""
import os
import sys
import time

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))

pytestmark = pytest.mark.gpu


def test_every_compiled_stage_instantiation_against_its_oracle():
    import torch

    import census
    import dsabeamformer_amd as bfm
    import stage_census
    from dsabeamformer_amd import api

    assert torch.cuda.is_available(), "these tests need a GPU"
    compiled = census.stage_compiled()
    rows = stage_census.ROWS
    assert {r.name for r in rows} == compiled and len(rows) == len(compiled)
    env = stage_census.Env(torch, bfm)
    seen, failures, lines, t_all, n_words = set(), [], [], time.perf_counter(), 0
    for row in rows:
        api.stage_launches(clear=True)
        t0, words, err = time.perf_counter(), 0, None
        try:
            words = row.run(env)                 # (compares with the oracle itself: bits, guard words)
        except AssertionError as e:              # a wrong bit is reported with the others; any other error ends the run here
            err = "differs from the oracle: %s" % (str(e)[:300].replace("\n", " "),)
        torch.cuda.synchronize()
        recorded = api.stage_launches(clear=True)
        seen |= set(recorded)
        if err is None and row.name not in recorded:
            err = "not launched: the call recorded %s" % sorted(set(recorded))
        if err is None and not words > 0:
            err = "nothing was compared"
        n_words += words
        lines.append("%-58s %-70s %9d words %8.3f s  %s" % (row.name, row.case, words, time.perf_counter() - t0, err or "ok"))
        if err:
            failures.append((row.name, row.case, err))
    total = time.perf_counter() - t_all
    report = ("# tests/test_gpu_stage_census.py: %d stage kernel instantiations on %d CUs, %d words compared, %d failures, %.1f s\n"
              % (len(rows), env.n_cus, n_words, len(failures), total) +
              "# %-56s %-70s %15s %10s\n" % ("kernel (as the launcher recorded it)", "case", "compared", "time") + "\n".join(lines) + "\n")
    print(report)
    if os.environ.get("DSABF_REPORT_DIR"):
        os.makedirs(os.environ["DSABF_REPORT_DIR"], exist_ok=True)
        with open(os.path.join(os.environ["DSABF_REPORT_DIR"], "stage_census_gpu.txt"), "w") as fp:
            fp.write(report)
    print("stage census: %d instantiations, %d words compared, %.1f s" % (len(rows), n_words, total))
    for name, case, err in failures:
        print("FAILED %s (%s): %s" % (name, case, err))
    assert not failures, [name for name, _, _ in failures]
    assert sorted(seen - compiled) == [], "recorded by a launcher, but not a kernel of the library"
    assert sorted(compiled - seen) == [], "compiled, but never launched"
