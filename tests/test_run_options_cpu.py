"""CPU test of run_observation's refusals (include/dsabf_host.hpp): every option combination the production loop turns down, with its
return code and its bf_last_error() text, before anything is read or created.  A small C++ program with its own main (the precedent
is tests/test_events_cpu.py::test_both_files_round_trip) builds a valid bf_config and observation_options, applies one mutation per
case and calls run_observation with a block_source whose every method aborts.  The five rules that need a live communicator (its
rank / world, the sharded gather's launches, the two "only the gather root" sinks, voltage cuts on a sharded run) are not here: a
bf_comm cannot exist without a device."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <iostream>
#include <sstream>

#include "dsabf_host.hpp"

using namespace dsabf;

// refusals come "before anything is read or created": a source that is touched ends the program
struct untouchable_source : block_source {
    void read_headers() override { abort(); }
    char* read() override { abort(); }
    void close() override { abort(); }
    bool check_transfers_complete() override { abort(); }
    uint64_t get_block_size() const override { abort(); }
    uint64_t get_bytes_read() const override { abort(); }
    bool close_releases_block() const override { abort(); }
};

// a sink that is only ever compared with NULL: a call through it has no object to land in
static long nothing[8];
template <class T> T* a_sink() { return reinterpret_cast<T*>(nothing); }

constexpr int kFreq = 4, kBeams = 8;
static int32_t delays[2 * kFreq];
static bf_evt_options evt_options;
static bf_psr_model psr_model = {0, 1, 0, 0};
static uint8_t mask[kFreq];

static void with_dm(observation_options& o) { o.dm_delays = delays; o.n_dm = 2; }
static void with_sps(observation_options& o) { with_dm(o); o.sps_widths = 3; }
static void with_evt(observation_options& o) { with_sps(o); o.evt = &evt_options; }
static void with_vcut(observation_options& o) { with_evt(o); o.vcut_sink = a_sink<voltage_sink>(); }
static void with_psr(observation_options& o) { with_dm(o); o.n_psr = 1; o.psr_models = &psr_model; o.psr_delays = delays; o.psr_dump_rows = 8; }

static inj_plan plan;   // what a case's opt.inj points at
static inj_plan::burst a_burst() { inj_plan::burst b; b.W = 2; b.delay.assign(kFreq, 0); b.profile.assign(kFreq * 2, 1.0f); b.response.assign(kBeams, 1.0f); return b; }
static inj_plan::train a_train() { inj_plan::train t; t.n_bins = 4; t.delay.assign(kFreq, 0); t.profile.assign(kFreq * 4, 1.0f); t.response.assign(kBeams, 1.0f); return t; }
static void with_inj(observation_options& o) { with_dm(o); plan = inj_plan(); o.inj = &plan; }

static void refuse(const char* name, const std::function<void(bf_config&, observation_options&)>& mutate)
{
    bf_config cfg;
    bf_config_default(&cfg, 0);
    cfg.n_beams = kBeams; cfg.n_ant = 8; cfg.n_freq = kFreq; cfg.n_avg = 16; cfg.n_out_per_gemm = 2; cfg.n_gemms_per_block = 4; cfg.n_streams = 2;
    observation_options opt;
    mutate(cfg, opt);
    untouchable_source source;
    std::ostringstream log;
    const int rc = run_observation(cfg, opt, source, nullptr, nullptr, nullptr, log);
    printf("%s|%d|%s|%s\n", name, rc, bf_last_error(), log.str().c_str());
}

int main()
{
    bf_evt_default_options(&evt_options);
    // the one refusal without a text of its own (the reference's static_assert): first, while the thread's error text is still untouched
    refuse("gemms_per_block_not_a_multiple_of_streams", [](bf_config& c, observation_options&) { c.n_gemms_per_block = 3; });
    refuse("world_0", [](bf_config&, observation_options& o) { o.world = 0; });
    refuse("rank_beyond_world", [](bf_config&, observation_options& o) { o.rank = 1; });
    refuse("rank_negative", [](bf_config&, observation_options& o) { o.rank = -1; });
    refuse("gather_root_beyond_world", [](bf_config&, observation_options& o) { o.gather_root = 1; });
    refuse("gather_root_below_all", [](bf_config&, observation_options& o) { o.gather_root = BF_GATHER_ROOT_ALL - 1; });
    refuse("dm_delays_without_n_dm", [](bf_config&, observation_options& o) { o.dm_delays = delays; });
    refuse("dm_sink_without_dm_delays", [](bf_config&, observation_options& o) { o.dm_sink = a_sink<dm_chunk_sink>(); });
    refuse("sps_widths_negative", [](bf_config&, observation_options& o) { with_dm(o); o.sps_widths = -1; });
    refuse("sps_widths_9", [](bf_config&, observation_options& o) { with_dm(o); o.sps_widths = 9; });
    refuse("sps_widths_without_dm_delays", [](bf_config&, observation_options& o) { o.sps_widths = 3; });
    refuse("sps_sink_without_widths", [](bf_config&, observation_options& o) { with_dm(o); o.sps_sink = a_sink<sps_candidate_sink>(); });
    refuse("evt_without_sps_widths", [](bf_config&, observation_options& o) { with_dm(o); o.evt = &evt_options; });
    refuse("event_sink_without_evt", [](bf_config&, observation_options& o) { with_sps(o); o.event_sink = a_sink<event_sink>(); });
    refuse("stamp_sink_without_evt", [](bf_config&, observation_options& o) { with_sps(o); o.stamp_sink = a_sink<stamp_sink>(); });
    refuse("stamp_bins_0", [](bf_config&, observation_options& o) { with_evt(o); o.stamp_bins = 0; });
    refuse("stamp_tbin_negative", [](bf_config&, observation_options& o) { with_evt(o); o.stamp_tbin = -1; });
    refuse("stamp_fbin_0", [](bf_config&, observation_options& o) { with_evt(o); o.stamp_fbin = 0; });
    refuse("stamp_fbin_not_dividing_the_band", [](bf_config&, observation_options& o) { with_evt(o); o.stamp_fbin = 3; });
    refuse("stamp_max_per_deliver_negative", [](bf_config&, observation_options& o) { with_evt(o); o.stamp_max_per_deliver = -1; });
    refuse("vcut_sink_without_evt", [](bf_config&, observation_options& o) { with_sps(o); o.vcut_sink = a_sink<voltage_sink>(); });
    refuse("vcut_units_0", [](bf_config&, observation_options& o) { with_vcut(o); o.vcut_units = 0; });
    refuse("vcut_history_units_negative", [](bf_config&, observation_options& o) { with_vcut(o); o.vcut_history_units = -1; });
    refuse("vcut_max_per_deliver_negative", [](bf_config&, observation_options& o) { with_vcut(o); o.vcut_max_per_deliver = -1; });
    refuse("cond_baseline_negative", [](bf_config&, observation_options& o) { with_dm(o); o.cond_baseline = -1; });
    refuse("cond_baseline_65", [](bf_config&, observation_options& o) { with_dm(o); o.cond_baseline = 65; });
    refuse("cond_baseline_without_dm_delays", [](bf_config&, observation_options& o) { o.cond_baseline = 4; });
    refuse("cond_mask_without_baseline", [](bf_config&, observation_options& o) { with_dm(o); o.cond_mask = mask; });
    refuse("cond_auto_threshold_without_baseline", [](bf_config&, observation_options& o) { with_dm(o); o.cond_auto_threshold = 3.0; });
    refuse("incoherent_beam_below_off", [](bf_config&, observation_options& o) { o.incoherent_beam = -2; });
    refuse("incoherent_beam_not_a_beam", [](bf_config&, observation_options& o) { o.incoherent_beam = kBeams; });
    refuse("corr_blocks_negative", [](bf_config&, observation_options& o) { o.corr_blocks = -1; });
    refuse("vis_sink_without_corr_blocks", [](bf_config&, observation_options& o) { o.vis_sink = a_sink<vis_sink>(); });
    refuse("corr_without_block_launch", [](bf_config&, observation_options& o) { o.corr_blocks = 2; o.block_launch = false; });
    refuse("n_psr_negative", [](bf_config&, observation_options& o) { with_psr(o); o.n_psr = -1; });
    refuse("n_psr_5", [](bf_config&, observation_options& o) { with_psr(o); o.n_psr = 5; });
    refuse("psr_without_dm_delays", [](bf_config&, observation_options& o) { with_psr(o); o.dm_delays = nullptr; o.n_dm = 0; });
    refuse("psr_without_models", [](bf_config&, observation_options& o) { with_psr(o); o.psr_models = nullptr; });
    refuse("psr_without_delays", [](bf_config&, observation_options& o) { with_psr(o); o.psr_delays = nullptr; });
    refuse("psr_bins_1", [](bf_config&, observation_options& o) { with_psr(o); o.psr_bins = 1; });
    refuse("psr_bins_4097", [](bf_config&, observation_options& o) { with_psr(o); o.psr_bins = 4097; });
    refuse("psr_dump_rows_0", [](bf_config&, observation_options& o) { with_psr(o); o.psr_dump_rows = 0; });
    refuse("psr_sink_without_n_psr", [](bf_config&, observation_options& o) { with_dm(o); o.psr_sink = a_sink<psr_sink>(); });
    refuse("inj_burst_without_dm_delays", [](bf_config&, observation_options& o) { with_inj(o); plan.bursts.push_back(a_burst()); o.dm_delays = nullptr; o.n_dm = 0; });
    refuse("inj_train_without_dm_delays", [](bf_config&, observation_options& o) { with_inj(o); plan.trains.push_back(a_train()); o.dm_delays = nullptr; o.n_dm = 0; });
    refuse("inj_burst_W_0", [](bf_config&, observation_options& o) { with_inj(o); plan.bursts.push_back(a_burst()); plan.bursts[0].W = 0; });
    refuse("inj_burst_delay_size", [](bf_config&, observation_options& o) { with_inj(o); plan.bursts.push_back(a_burst()); plan.bursts[0].delay.pop_back(); });
    refuse("inj_burst_profile_size", [](bf_config&, observation_options& o) { with_inj(o); plan.bursts.push_back(a_burst()); plan.bursts[0].profile.pop_back(); });
    refuse("inj_burst_response_size", [](bf_config&, observation_options& o) { with_inj(o); plan.bursts.push_back(a_burst()); plan.bursts[0].response.pop_back(); });
    refuse("inj_train_n_bins_1", [](bf_config&, observation_options& o) { with_inj(o); plan.trains.push_back(a_train()); plan.trains[0].n_bins = 1; });
    refuse("inj_train_delay_size", [](bf_config&, observation_options& o) { with_inj(o); plan.trains.push_back(a_train()); plan.trains[0].delay.pop_back(); });
    refuse("inj_train_profile_size", [](bf_config&, observation_options& o) { with_inj(o); plan.trains.push_back(a_train()); plan.trains[0].profile.pop_back(); });
    refuse("inj_train_response_size", [](bf_config&, observation_options& o) { with_inj(o); plan.trains.push_back(a_train()); plan.trains[0].response.pop_back(); });
    refuse("inj_more_bursts_than_pulses", [](bf_config&, observation_options& o) { with_inj(o); plan.bursts.assign((size_t)BF_INJ_MAX_PULSES + 1, a_burst()); });
    refuse("inj_more_trains_than_trains", [](bf_config&, observation_options& o) { with_inj(o); plan.trains.assign((size_t)BF_INJ_MAX_TRAINS + 1, a_train()); });
    refuse("ffa_p_hi_negative", [](bf_config&, observation_options& o) { with_dm(o); o.ffa_p_hi = -1; });
    refuse("ffa_without_dm_delays", [](bf_config&, observation_options& o) { o.ffa_p_lo = 8; o.ffa_p_hi = 13; });
    refuse("ffa_sink_without_p_hi", [](bf_config&, observation_options& o) { with_dm(o); o.ffa_sink = a_sink<ffa_sink>(); });
    refuse("sk_blocks_negative", [](bf_config&, observation_options& o) { o.sk_blocks = -1; });
    refuse("sk_sink_without_sk_blocks", [](bf_config&, observation_options& o) { o.sk_sink = a_sink<sk_sink>(); });
    refuse("sk_without_block_launch", [](bf_config&, observation_options& o) { o.sk_blocks = 2; o.block_launch = false; });
    refuse("stokes_sink_without_beams", [](bf_config&, observation_options& o) { o.stokes_sink = a_sink<stokes_sink>(); });
    refuse("stokes_int_without_beams", [](bf_config&, observation_options& o) { o.stokes_int = 4; });
    refuse("stokes_without_block_launch", [](bf_config&, observation_options& o) { o.stokes_beams = {0}; o.block_launch = false; });
    refuse("stokes_17_beams", [](bf_config&, observation_options& o) { o.stokes_beams.assign((size_t)BF_STOKES_MAX_BEAMS + 1, 0); });
    refuse("stokes_beam_negative", [](bf_config&, observation_options& o) { o.stokes_beams = {0, -1}; });
    refuse("stokes_beam_not_a_beam", [](bf_config&, observation_options& o) { o.stokes_beams = {0, kBeams}; });
    refuse("stokes_int_not_dividing", [](bf_config&, observation_options& o) { o.stokes_beams = {0}; o.stokes_int = 3; });
    refuse("stokes_int_negative", [](bf_config&, observation_options& o) { o.stokes_beams = {0}; o.stokes_int = -1; });
    refuse("dm_split_trials_without_comm", [](bf_config&, observation_options& o) { with_dm(o); o.dm_split_trials = true; });
    // two rules of one stage broken at once: which message wins
    refuse("both_sps_sink_without_dm_delays_and_without_widths", [](bf_config&, observation_options& o) { o.sps_sink = a_sink<sps_candidate_sink>(); });
    refuse("both_evt_without_sps_widths_and_stamp_bins_0", [](bf_config&, observation_options& o) { with_dm(o); o.evt = &evt_options; o.stamp_bins = 0; });
    refuse("both_corr_blocks_negative_and_no_block_launch", [](bf_config&, observation_options& o) { o.corr_blocks = -1; o.block_launch = false; });
    refuse("both_stokes_17_beams_and_no_block_launch", [](bf_config&, observation_options& o) { o.stokes_beams.assign(17, 0); o.block_launch = false; });
    refuse("both_psr_without_dm_delays_and_without_models", [](bf_config&, observation_options& o) { o.n_psr = 1; });
    return 0;
}
"""

INVALID = -1
NEEDS_DM = "run_observation: %s needs the DM stage (dm_delays)"
RANKS = "run_observation: need 0 <= rank < world and gather_root a rank or BF_GATHER_ROOT_ALL"
STAMPS = "run_observation: need stamp_bins >= 1, stamp_tbin >= 0, stamp_max_per_deliver >= 0 and stamp_fbin >= 1 dividing the band"
VCUTS = "run_observation: need vcut_units >= 1, vcut_history_units >= 0 and vcut_max_per_deliver >= 0"
BURST = "run_observation: an injected burst needs W >= 1, delay [band], profile [band][W] and response [n_beams]"
TRAIN = "run_observation: an injected train needs n_bins >= 2, delay [band], profile [band][n_bins] and response [n_beams]"
PLAN = "run_observation: the injection plan holds more than BF_INJ_MAX_TRAINS trains or BF_INJ_MAX_PULSES pulses"
PSR_SHAPE = "run_observation: the pulsar folder needs psr_bins in 2 .. 4096 and psr_dump_rows >= 1"

# (case, return code, bf_last_error()): the parent commit's output, in the program's order
REFUSALS = [
    ("gemms_per_block_not_a_multiple_of_streams", INVALID, ""),
    ("world_0", INVALID, RANKS),
    ("rank_beyond_world", INVALID, RANKS),
    ("rank_negative", INVALID, RANKS),
    ("gather_root_beyond_world", INVALID, RANKS),
    ("gather_root_below_all", INVALID, RANKS),
    ("dm_delays_without_n_dm", INVALID, "run_observation: dm_delays without n_dm"),
    ("dm_sink_without_dm_delays", INVALID, "run_observation: a dm_sink needs dm_delays"),
    ("sps_widths_negative", INVALID, "run_observation: sps_widths must be 0 (off) .. 8"),
    ("sps_widths_9", INVALID, "run_observation: sps_widths must be 0 (off) .. 8"),
    ("sps_widths_without_dm_delays", INVALID, NEEDS_DM % "the single-pulse search"),
    ("sps_sink_without_widths", INVALID, "run_observation: a sps_sink needs sps_widths > 0"),
    ("evt_without_sps_widths", INVALID, "run_observation: the event builder (evt) needs sps_widths > 0"),
    ("event_sink_without_evt", INVALID, "run_observation: an event_sink or a stamp_sink needs evt"),
    ("stamp_sink_without_evt", INVALID, "run_observation: an event_sink or a stamp_sink needs evt"),
    ("stamp_bins_0", INVALID, STAMPS),
    ("stamp_tbin_negative", INVALID, STAMPS),
    ("stamp_fbin_0", INVALID, STAMPS),
    ("stamp_fbin_not_dividing_the_band", INVALID, STAMPS),
    ("stamp_max_per_deliver_negative", INVALID, STAMPS),
    ("vcut_sink_without_evt", INVALID, "run_observation: a vcut_sink needs evt"),
    ("vcut_units_0", INVALID, VCUTS),
    ("vcut_history_units_negative", INVALID, VCUTS),
    ("vcut_max_per_deliver_negative", INVALID, VCUTS),
    ("cond_baseline_negative", INVALID, "run_observation: cond_baseline must be 0 (off) .. 64"),
    ("cond_baseline_65", INVALID, "run_observation: cond_baseline must be 0 (off) .. 64"),
    ("cond_baseline_without_dm_delays", INVALID, NEEDS_DM % "the conditioner"),
    ("cond_mask_without_baseline", INVALID, "run_observation: cond_mask / cond_auto_threshold need cond_baseline > 0"),
    ("cond_auto_threshold_without_baseline", INVALID, "run_observation: cond_mask / cond_auto_threshold need cond_baseline > 0"),
    ("incoherent_beam_below_off", INVALID, "run_observation: incoherent_beam must be -1 (off) or a beam index"),
    ("incoherent_beam_not_a_beam", INVALID, "run_observation: incoherent_beam must be -1 (off) or a beam index"),
    ("corr_blocks_negative", INVALID, "run_observation: corr_blocks must be 0 (off) or the blocks per dump"),
    ("vis_sink_without_corr_blocks", INVALID, "run_observation: a vis_sink needs corr_blocks > 0"),
    ("corr_without_block_launch", INVALID, "run_observation: the correlator needs block-granular launches"),
    ("n_psr_negative", INVALID, "run_observation: n_psr must be 0 (off) .. 4"),
    ("n_psr_5", INVALID, "run_observation: n_psr must be 0 (off) .. 4"),
    ("psr_without_dm_delays", INVALID, NEEDS_DM % "the pulsar folder"),
    ("psr_without_models", INVALID, "run_observation: n_psr > 0 needs psr_models and psr_delays"),
    ("psr_without_delays", INVALID, "run_observation: n_psr > 0 needs psr_models and psr_delays"),
    ("psr_bins_1", INVALID, PSR_SHAPE),
    ("psr_bins_4097", INVALID, PSR_SHAPE),
    ("psr_dump_rows_0", INVALID, PSR_SHAPE),
    ("psr_sink_without_n_psr", INVALID, "run_observation: a psr_sink needs n_psr > 0"),
    ("inj_burst_without_dm_delays", INVALID, NEEDS_DM % "pulse injection"),
    ("inj_train_without_dm_delays", INVALID, NEEDS_DM % "pulse injection"),
    ("inj_burst_W_0", INVALID, BURST),
    ("inj_burst_delay_size", INVALID, BURST),
    ("inj_burst_profile_size", INVALID, BURST),
    ("inj_burst_response_size", INVALID, BURST),
    ("inj_train_n_bins_1", INVALID, TRAIN),
    ("inj_train_delay_size", INVALID, TRAIN),
    ("inj_train_profile_size", INVALID, TRAIN),
    ("inj_train_response_size", INVALID, TRAIN),
    ("inj_more_bursts_than_pulses", INVALID, PLAN),
    ("inj_more_trains_than_trains", INVALID, PLAN),
    ("ffa_p_hi_negative", INVALID, "run_observation: ffa_p_hi must be 0 (off) or the end of the period range"),
    ("ffa_without_dm_delays", INVALID, NEEDS_DM % "the periodicity search"),
    ("ffa_sink_without_p_hi", INVALID, "run_observation: an ffa_sink needs ffa_p_hi > 0"),
    ("sk_blocks_negative", INVALID, "run_observation: sk_blocks must be 0 (off) or the blocks per dump"),
    ("sk_sink_without_sk_blocks", INVALID, "run_observation: a sk_sink needs sk_blocks > 0"),
    ("sk_without_block_launch", INVALID, "run_observation: the voltage moments need block-granular launches"),
    ("stokes_sink_without_beams", INVALID, "run_observation: a stokes_sink / stokes_int needs stokes_beams"),
    ("stokes_int_without_beams", INVALID, "run_observation: a stokes_sink / stokes_int needs stokes_beams"),
    ("stokes_without_block_launch", INVALID, "run_observation: the Stokes beams need block-granular launches"),
    ("stokes_17_beams", INVALID, "run_observation: stokes_beams holds more than BF_STOKES_MAX_BEAMS beams"),
    ("stokes_beam_negative", INVALID, "run_observation: a stokes_beams index is not a beam"),
    ("stokes_beam_not_a_beam", INVALID, "run_observation: a stokes_beams index is not a beam"),
    ("stokes_int_not_dividing", INVALID, "run_observation: stokes_int must divide n_out_per_gemm * n_avg"),
    ("stokes_int_negative", INVALID, "run_observation: stokes_int must divide n_out_per_gemm * n_avg"),
    ("dm_split_trials_without_comm", INVALID, "run_observation: dm_split_trials needs a sharded run gathered to every rank (BF_GATHER_ROOT_ALL)"),
    ("both_sps_sink_without_dm_delays_and_without_widths", INVALID, NEEDS_DM % "the single-pulse search"),
    ("both_evt_without_sps_widths_and_stamp_bins_0", INVALID, "run_observation: the event builder (evt) needs sps_widths > 0"),
    ("both_corr_blocks_negative_and_no_block_launch", INVALID, "run_observation: corr_blocks must be 0 (off) or the blocks per dump"),
    ("both_stokes_17_beams_and_no_block_launch", INVALID, "run_observation: the Stokes beams need block-granular launches"),
    ("both_psr_without_dm_delays_and_without_models", INVALID, NEEDS_DM % "the pulsar folder"),
]


@pytest.fixture(scope="module")
def refusals(tmp_path_factory):
    """The program's output, one (code, error text, log) per case name: compiled and run once."""
    from dsabeamformer_amd import build as b

    b.build()
    tmp = tmp_path_factory.mktemp("run_options")
    src, exe = tmp / "refusals.cpp", tmp / "refusals"
    src.write_text(PROGRAM)
    pkg = os.path.dirname(b.LIB)
    hip_lib = os.path.join(os.path.dirname(os.path.realpath(b.HIPCC)), "..", "lib")   # the library leaves its hip* symbols to the application
    r = subprocess.run([shutil.which("g++") or "g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L" + pkg, "-ldsabf", "-L" + hip_lib, "-lamdhip64", "-Wl,-rpath," + pkg, "-Wl,-rpath," + hip_lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])   # (an abort: a refusal came too late, the source was touched)
    out = {}
    for line in r.stdout.splitlines():
        name, code, text, log = line.split("|")
        assert name not in out, name
        out[name] = (int(code), text, log)
    return out


def test_every_case_ran_once(refusals):
    assert list(refusals) == [name for name, _, _ in REFUSALS]


@pytest.mark.parametrize("name,code,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(refusals, name, code, text):
    """The code and the text, and nothing logged: a refusal comes before the first line of the run."""
    assert refusals[name] == (code, text, "")
