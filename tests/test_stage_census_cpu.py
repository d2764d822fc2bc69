"""The census of the stage kernels, CPU side: the table of tests/support/stage_census.py claims exactly the instantiations of
csrc/<stage>/ that are compiled into libdsabf.so (tools/census.py::stage_compiled) -- a row too few is an instantiation no GPU test
is bound to launch, a row too many a kernel that is gone --, and every launch site of those directories records the kernel it is
about to launch (csrc/rec/bf_launch_record.h), which is what tests/test_gpu_stage_census.py reads back."""
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import census  # noqa: E402
import stage_census  # noqa: E402


@pytest.fixture(scope="module")
def compiled():
    from dsabeamformer_amd import build

    build.build()
    return census.stage_compiled()


def test_the_table_claims_the_compiled_set(compiled):
    claimed = [r.name for r in stage_census.ROWS]
    assert len(claimed) == len(set(claimed)), sorted(n for n in set(claimed) if claimed.count(n) > 1)
    assert sorted(compiled - set(claimed)) == [], "compiled, but no row of tests/support/stage_census.py launches them"
    assert sorted(set(claimed) - compiled) == [], "claimed by a row, but not in the library"
    # the templates the launchers switch over, counted: a template that loses an instantiation shows here by name
    count = lambda prefix: len([k for k in compiled if k.startswith(prefix)])
    assert (count("stokes_kernel<"), count("cdd_kernel<"), count("incoherent_kernel<"), count("sps_tile_kernel<"), count("ffa_search_kernel<"),
            count("psr_fold_kernel<"), count("inj_burst_kernel<"), count("inj_train_kernel<"), count("rm_kernel<")) == (32, 14, 8, 8, 6, 4, 4, 4, 3)
    assert all(r.case and callable(r.run) for r in stage_census.ROWS)


def test_stage_kernels_are_not_counted_among_the_others(compiled):
    others = set(census.other_kernels())
    assert not others & compiled and not [k for k in others if re.match(r"fused(?:16|g)_kernel<", k)]
    assert {"dedisperse_dm_kernel", "dedisperse_dm_wide_kernel", "expand_kernel"} <= others
    assert census.stage_kernel_names() == {k.split("<")[0] for k in compiled}, "a __global__ of csrc/<stage>/ that is not in the library, or the reverse"


def test_every_launch_site_records_its_kernel():
    """In every .hip file of the stage directories: as many record calls as launch sites, each record directly in front of its launch
    (same statement line or the line above), so a new launch site cannot forget one."""
    sources = census.stage_sources()
    assert {os.path.basename(os.path.dirname(p)) for p in sources} == set(census.STAGE_DIRS)
    total = 0
    for path in sources:
        lines = open(path).read().split("\n")
        launches = [i for i, l in enumerate(lines) if "hipLaunchKernelGGL(" in l or "<<<" in l]
        records = [i for i, l in enumerate(lines) if re.search(r"\brecord_launchf?\(", l)]
        assert len(launches) == len(records) > 0, (path, len(launches), len(records))
        for i in launches:
            assert i in records or i - 1 in records, "%s:%d launches without recording the kernel in front of it" % (path, i + 1)
        total += len(launches)
    assert total >= len(census.STAGE_DIRS)
    assert '#include "dsabf_bench.h"' in open(os.path.join(ROOT, "dsabeamformer_amd", "csrc", "rec", "bf_launch_record.cpp")).read()


def test_the_record_is_empty_without_a_launch_and_the_entry_point_refuses_a_small_buffer():
    import ctypes as C

    from dsabeamformer_amd import api, load

    assert api.stage_launches(clear=True) == [] and api.stage_launches() == []
    assert load().bf_stage_launches(None, 10, 0) != 0 and load().bf_stage_launches(C.create_string_buffer(4), 0, 0) != 0
