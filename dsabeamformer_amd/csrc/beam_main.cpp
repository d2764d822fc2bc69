// beam_main.cpp -- the `beam` driver: command line and lifecycle of the reference's main() (src/beamformer.cu:12-157,
// 539-571; usage() src/beamformer.hh:222-243) on top of libdsabf.so.
//
//   beam [-g gpu] [-p position_file] [-d direction_file] [-s source_file] [-o data.py] [-D device] [-a n_avg] [-u] [-v] [-h | -H]
//        (-u: the reference's launch pattern, one launch + copy per gemm-unit, instead of one per block; same data.py)
//   beam -j n_blocks [-g gpu] [-p ...] [-d ...]     production geometry, observation loop fed by the in-memory
//                                                   dada_junkdb stand-in (soak / data-rate run, makefile:28-29)
//   beam -j n_blocks -R world -r rank -I idfile     one frequency SHARD of a sub-band: this process beamforms channels
//                                                   [rank * 256/world, (rank+1) * 256/world); after every block the
//                                                   shards' detected powers are gathered to rank 0 (RCCL over xGMI), which
//                                                   alone writes -w / -K.  idfile: rank 0 publishes the 128-byte RCCL
//                                                   unique id there, the others wait for it.  beam_replicas -S starts
//                                                   the `world` processes.  (The reference's own scaling -- 8 independent
//                                                   sub-bands selected by -g, README.md:168 -- is beam_replicas without -S.)
//   beam -j n_blocks -M dm_max [-N n_dm] [-T tsamp_ms] [-W dm_file | -Q dm_ring]
//                                                   the DM stage, where the reference's loop has its DM-0
//                                                   collapse (src/beamformer.cu:492-511): the ladder of sandbox/Dispersion
//                                                   Theory.ipynb from 0 to dm_max (at most n_dm of its trials, evenly picked),
//                                                   every analysed block through a bf_dm_stream with the delay window carried
//                                                   over on the device, chunks [dm][t][beam] to dm_file.  With -R: on the
//                                                   gather root, over the gathered band.  With -R and -X: the shards' powers go to
//                                                   EVERY rank (the one collective becomes an all-gather) and rank r dedisperses its
//                                                   share of the ladder, writing dm_file.<r>: the DM work scales with the GPUs.
//   beam -j n_blocks -M dm_max ... -S snr [-B n_widths] [-C cand_file]
//                                                   the single-pulse search behind the DM stage (docs/SINGLE_PULSE.md): every chunk
//                                                   searched on the device with boxcar widths 1 .. 2^(n_widths-1) [6]; candidates at
//                                                   S/N >= snr to cand_file, one text line each: t_start dm beam width snr peak.
//                                                   With -X: cand_file.<r>, trials numbered over the whole ladder.  Needs -M.
//   beam -j n_blocks -M dm_max ... -n baseline_pushes [-z] [-U auto_threshold] [-F mask_file]
//                                                   the conditioner in front of the DM stage (docs/CONDITIONING.md): every analysed block
//                                                   normalised per (channel, beam) against the last baseline_pushes blocks and masked, in
//                                                   the DM stage's buffer (-w / -K keep the raw stream).  -z: also subtract the mean over
//                                                   the unmasked channels per (time, beam) (off here unless given); -U: mask channels whose
//                                                   cv / cm^2 lies more than auto_threshold scaled median deviations above the median;
//                                                   -F: a text file of channel indices to mask, one per line, # comments.  Needs -M.
//   beam -j n_blocks ... -i beam                    the incoherent beam (docs/INCOHERENT_BEAM.md): beam column `beam` of the detected
//                                                   stream carries the antenna powers summed over the antennas instead of a tied beam,
//                                                   for -w / -K, the DM stage and the search alike.  With -R: every shard, same index.
//   beam -j n_blocks ... -V vis_file [-L corr_blocks]
//                                                   the correlator (docs/CORRELATOR.md): the antenna visibilities of every analysed
//                                                   block, integrated over corr_blocks blocks [1] per dump, to vis_file (int64 lower
//                                                   triangle per channel and polarisation).  With -R: every shard correlates its own
//                                                   channels and writes vis_file.<rank>.  (-j counts the 25 burn-in reads: -j 27
//                                                   analyses two blocks.)
//   beam -E vis_file -G gains_file [-P]            the gain solver (docs/CALIBRATION.md), no observation: every record of a file written
//                                                   by -V is solved for the per-(channel, polarisation, antenna) gains of a calibrator at
//                                                   the phase centre (-P: the polarisations jointly, one layer) and written as one record
//                                                   of gains_file; the geometry comes from vis_file's header (a shard's vis_file.<rank> too).
//   beam ... -A gains_file                          DEBUG run or observation mode: layer 0 of the last record of gains_file calibrates the
//                                                   steering weights (conj(g) / |g|) before they are set.
//   beam -j n_blocks ... -Y moments_file [-J sk_blocks]
//                                                   the voltage moments (docs/SPECTRAL_KURTOSIS.md): sum |v|^2 and sum |v|^4 per (channel,
//                                                   polarisation, antenna) of every analysed block, integrated over sk_blocks blocks [1] per
//                                                   dump, to moments_file.  With -R: every shard its own channels, moments_file.<rank>.
//   beam -e moments_file -O ant_file [-q chan_file] [-t n_sigma] [-m centre]
//                                                   select mode, no device: the records of a -Y file summed, the spectral-kurtosis rule
//                                                   (bf_sk_select, defaults centre 1, 5 sigma) applied, the flagged antennas to ant_file and
//                                                   the flagged channels to chan_file, both in the -F format (chan_file can be given to -F).
//   beam -j n_blocks ... -x stokes_file -b b0,b1,... [-l n_int]
//                                                   full-Stokes follow-up beams (docs/STOKES.md): I, Q, U, V as exact int64 of up to 16
//                                                   of the beams, summed over windows of n_int samples [N_AVERAGING; 1 = every voltage
//                                                   sample], one record per launch, to stokes_file.  With -R: stokes_file.<rank>.
//   beam -E vis_file -G gains_file -f ant_file     the solver leaves the listed antennas out (their gains are exactly zero);
//   beam ... -A gains_file -f ant_file              the listed antennas get zero weights.
//   beam -E vis_file -Z null_file [-y n_null[:min_ratio]] [-f ant_file]
//                                                   the spatial null (docs/NULLING.md), no observation: the dominant eigenvectors of every
//                                                   record of a -V file (up to n_null [1] per channel, each used only if it stands min_ratio [4]
//                                                   above the rest) written as one record of null_file.  -G may be given in the same run.
//                                                   With -R world -r rank: vis_file.<rank> -> null_file.<rank>.
//   beam ... -Z null_file [-f ant_file]             DEBUG run or observation mode: the vectors of the last record of null_file are projected
//                                                   out of the steering weights before they are set (after -A's gains; -x follows the same
//                                                   weights).  With -R: null_file.<rank>.
//
// With the reference's `make debug` geometry (default) it generates synthetic point-source voltages on the CPU,
// streams them through the observation loop and writes bin/data.py (dedispersed beam responses, one row per source)
// exactly like the reference's DEBUG build.  The PSRDADA observation mode (-c core, -k key) needs libpsrdada, which is
// not part of this build; the options are accepted and reported.
#include <fcntl.h>
#include <getopt.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <fstream>
#include <thread>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/dsabf_host.hpp"

namespace {
using namespace dsabf;

// ---------------------------------------------------------------------------------------------------------------------------------
// What the command line says, one group per stage.  `given`: an option of the group other than its main one appeared; `bad`: one of
// its numbers was malformed.  parse() fills it, check() judges it, nothing changes it afterwards.
// ---------------------------------------------------------------------------------------------------------------------------------
struct fold_spec {
    double f0 = 0.0, f1 = 0.0, phase0 = 0.0;
};
struct inject_spec {
    double v[6] = {0, 0, 0, 0, 0, 0};   // t0|f0 dm beam fluence|amp sigma|duty w|bins
    int n = 0;                          // fields given
};

struct options {
    bf_config cfg;           // the DEBUG geometry: -a, -v
    debug_run_options run;   // -g, -D, -v
    bool per_unit = false;   // -u
    std::string positions, directions, sources, output = "bin/data.py";   // -p -d -s -o
    // observation mode: -j blocks of the in-memory source, or -k ring [-c core]; -w file / -K ring keep the detected stream
    long junk_blocks = -1;
    std::string ring_key, detected_path, out_ring;
    int core = -1;
    bool observe() const { return junk_blocks >= 0 || !ring_key.empty(); }
    struct {   // -R world -r rank -I idfile
        int world = 1, rank = 0;
        std::string id_file;
    } shard;
    struct {   // -M dm_max [-N n_dm] [-T tsamp_ms] [-W file | -Q ring] [-X]
        double max = 0.0, tsamp_ms = 0.131;   // (the notebook's sample time, cell 5)
        int cap = 0;
        bool split = false;
        std::string path, ring;
        bool on() const { return max > 0.0; }
    } dm;
    struct {   // -S snr [-B n_widths] [-C cand_file]
        bool on = false, widths_given = false;
        double snr = 0.0;
        int widths = 6;
        std::string cand_path;
    } sps;
    struct {   // -n baseline_pushes [-z] [-U auto_threshold] [-F mask_file]
        bool given = false, zero_dm = false, auto_given = false;
        int pushes = 0;
        double auto_threshold = 0.0;
        std::string mask_path;
    } cond;
    struct {   // -i beam
        bool given = false;
        int beam = -1;
    } ib;
    struct blocks_to_file {   // -V vis_file [-L corr_blocks]; -Y moments_file [-J sk_blocks]
        std::string path;
        int blocks = 1;
        bool blocks_given = false;
    } corr, sk;
    struct {   // -E vis_file -G gains_file [-P]; -A gains_file; -f ant_file
        std::string vis, gains_path, apply, ant_flags_path;
        bool joint = false;
    } solve;
    struct {   // -Z null_file [-y n_null[:min_ratio]]
        std::string path, spec;
        bool bad = false;
        bf_null_options opt;
    } null;
    struct {   // -e moments_file -O ant_file [-q chan_file] [-t n_sigma] [-m centre]
        std::string path, ant_path, chan_path;
        bf_sk_options opt;
        bool given = false;
    } select;
    struct {   // -x stokes_file -b b0,b1,... [-l n_int]
        std::string path, list;
        int n_int = 0;   // 0: N_AVERAGING
        bool int_given = false;
        std::vector<int> beams;   // check() parses -b against the production band
    } stokes;
    struct {   // --events FILE [--event-tol T[,D]] [--event-veto MAXBEAMS[:IB_RATIO]]; --stamps FILE [--stamp-shape BINS[:TBIN[:FBIN]]] [--stamp-flagged]
        std::string path, stamps_path;
        bf_evt_options opt;
        int stamp_bins = 64, stamp_tbin = 0, stamp_fbin = 1;
        bool given = false, shape_given = false, stamp_flagged = false, bad = false;
    } evt;
    struct {   // --voltages FILE [--voltage-units N] [--voltage-history UNITS] [--voltage-flagged]
        std::string path;
        int units = 2, history = 0;
        bool given = false, flagged = false, bad = false;
    } vcut;
    struct {   // --coherent V_FILE --coherent-out FILE [--coherent-fft N] [--coherent-int n] [--coherent-sideband +1|-1]
        std::string path, out;
        int fft = 0, n_int = 1, sideband = 1;
        bool given = false, bad = false;
    } coherent;
    struct {   // --faraday C_FILE --faraday-out FILE [--faraday-phi lo:hi:n] [--faraday-window rows] [-F mask_file]
        std::string path, out;
        double phi_lo = 0.0, phi_hi = 0.0;
        int n_phi = 0, window = 0;   // 0: the default grid; 0: the record's search width
        bool given = false, phi_given = false, bad = false;
    } faraday;
    struct {   // --fold f0[:f1[:phase0]] (up to 4) [--fold-dm dm, the k-th for the k-th --fold] [--fold-bins n] [--fold-rows rows] [--fold-out FILE]
        std::vector<fold_spec> pulsars;
        std::vector<double> dms;
        int bins = 64, rows = 0;
        std::string path;
        bool given = false, bad = false;
    } fold;
    struct {   // --ffa p_lo:p_hi [--ffa-seg n] [--ffa-dec n] [--ffa-oct n] [--ffa-widths K] [--ffa-snr snr] [--ffa-out FILE] [--ffa-detrend blk:win]
        int p_lo = 0, p_hi = 0, seg = 1024, dec = 1, oct = 1, widths = 3, detrend_blk = 0, detrend_win = 0;
        double snr = 8.0;
        std::string path;
        bool on = false, given = false, bad = false;
    } ffa;
    struct {   // --inject t0:dm:beam:fluence[:sigma[:w]] (any number) [--inject-train f0:dm:beam:amp[:duty[:bins]]] (up to 4) [--inject-out FILE]
        std::vector<inject_spec> bursts, trains;
        std::string path;
        bool bad = false;
        bool on() const { return !bursts.empty() || !trains.empty(); }
    } inj;

    options()
    {
        bf_config_default(&cfg, /*debug=*/1);
        bf_sk_default_options(&select.opt);
        bf_null_default_options(&null.opt);
        bf_evt_default_options(&evt.opt);
    }
};

// the production geometry: the band of every observation, whatever -R
const bf_config& production_band()
{
    static const bf_config band = [] {
        bf_config c;
        bf_config_default(&c, /*debug=*/0);
        return c;
    }();
    return band;
}

// prints `beam: ...` and yields the exit status of a refused command line
__attribute__((format(printf, 1, 2))) int refuse(const char* fmt, ...)
{
    va_list args;
    va_start(args, fmt);
    fputs("beam: ", stderr);
    vfprintf(stderr, fmt, args);
    fputc('\n', stderr);
    va_end(args);
    return EXIT_FAILURE;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Fields of the long options
// ---------------------------------------------------------------------------------------------------------------------------------

// A whole number in [lo, hi] at the head of `text`; a first character out of `refused_lead` (a sign, a blank) refuses.  *end: what follows it.
bool whole(const char* text, long lo, long hi, const char* refused_lead, int* out, const char** end)
{
    char* e = nullptr;
    const long v = strtol(text, &e, 10);
    *out = (int)v;
    *end = e;
    return e != text && v >= lo && v <= hi && !strchr(refused_lead, *text);
}

// One to `max` whole numbers in [0, 1e9] without sign or leading blank, separated by `sep`, that fill `text`: how many, or -1.
int counts(const char* text, char sep, int max, int* const* out)
{
    for (int n = 0;;) {
        const char* end = nullptr;
        if (n == max || !whole(text, 0, 1000000000L, "-+ ", out[n], &end)) return -1;
        n++;
        if (!*end) return n;
        if (*end != sep) return -1;
        text = end + 1;
    }
}

// One to `max` numbers separated by colons that fill `text`: how many, or -1.
int reals(const char* text, int max, bool finite, double* out)
{
    for (int n = 0;;) {
        char* end = nullptr;
        if (n == max) return -1;
        out[n] = strtod(text, &end);
        if (end == text || (finite && !std::isfinite(out[n]))) return -1;
        n++;
        if (!*end) return n;
        if (*end != ':') return -1;
        text = end + 1;
    }
}

// a number that fills `text`
bool real(const char* text, double* out)
{
    char* end = nullptr;
    *out = strtod(text, &end);
    return end != text && !*end;
}

// The defaults of a pulse's optional fields, and the ranges that need no geometry: whole numbers where whole numbers go, DM >= 0,
// SIGMA > 0, W and BINS within the stage's bounds.
bool complete_pulse(inject_spec& sp, bool train)
{
    auto whole_in = [](double v, double lo, double hi) { return v >= lo && v <= hi && v == std::floor(v); };
    if (train) {
        if (sp.n < 5) sp.v[4] = 0.05;
        if (sp.n < 6) sp.v[5] = 64.0;
        return sp.v[1] >= 0.0 && whole_in(sp.v[2], 0, 1e9) && sp.v[4] > 0.0 && sp.v[4] <= 1.0 && whole_in(sp.v[5], 2, BF_PSR_MAX_BINS);
    }
    if (sp.n < 5) sp.v[4] = 1.0;
    if (sp.n < 6) {
        double w = 1.0;
        while (w < 8.0 * sp.v[4] && w <= (double)BF_INJ_MAX_WIDTH) w *= 2.0;
        sp.v[5] = w;
    }
    return whole_in(sp.v[0], 0, 9e15) && sp.v[1] >= 0.0 && whole_in(sp.v[2], 0, 1e9) && sp.v[4] > 0.0 && whole_in(sp.v[5], 1, BF_INJ_MAX_WIDTH);
}

// -H: the reference's text, then what this build adds to its command line
void extended_usage()
{
    usage(true, std::cout);
    std::cout << "extensions of this build (no counterpart in the reference):\n"
                 " -o file                 where the DEBUG run writes its table [bin/data.py]\n"
                 " -D device               HIP device index [0]\n"
                 " -a n_avg                N_AVERAGING of the DEBUG geometry [1]\n"
                 " -u                      the reference's launch pattern: one launch + copy per gemm-unit\n"
                 " -v                      verbose (the reference's -DVERBOSE)\n"
                 " -j n_blocks             observation mode: production geometry, in-memory dada_junkdb source\n"
                 " -k name | hexkey        observation mode: blocks from a shared-memory ring (hex key: PSRDADA builds)\n"
                 " -c core                 bind to a CPU core (with -k)\n"
                 " -w file | -K ring       keep the detected stream: file, or shared-memory ring to another process\n"
                 " -R world -r rank -I id  one frequency shard of a sub-band; powers gathered to rank 0 (RCCL)\n"
                 " -M dm_max [-N n_dm] [-T tsamp_ms]   the DM-trial stage inside the loop (notebook ladder 0 .. dm_max)\n"
                 " -W file | -Q ring       its chunks [dm][t][beam]: file of records, or shared-memory ring\n"
                 " -X                      with -R: gather to every shard, shard r dedisperses its share of the trials\n"
                 " -S snr [-B n_widths] [-C file]   single-pulse search of every DM chunk: boxcar widths 1 .. 2^(n_widths-1) [6],\n"
                 "                         candidates at S/N >= snr to file (t_start dm beam width snr peak; with -X: file.<rank>);\n"
                 "                         requires -M: without it (or -B / -C without -S) beam exits with a usage error\n"
                 " -n baseline_pushes [-z] [-U auto_threshold] [-F mask_file]   the conditioner in front of the DM stage: every block\n"
                 "                         normalised per (channel, beam) against the last baseline_pushes blocks (1 .. 64) and masked, in\n"
                 "                         the DM stage's buffer (-w / -K keep the raw stream); -z: zero-DM, the mean over the unmasked\n"
                 "                         channels subtracted per (time, beam); -U: automatic mask at auto_threshold scaled median\n"
                 "                         deviations; -F: channel indices to mask, one per line, # comments; requires -M, and -z / -U / -F\n"
                 "                         require -n: otherwise beam exits with a usage error\n"
                 "                         (with -z the ladder's DM-0 trial sums to the subtraction's rounding residue: its candidates,\n"
                 "                         S/N 7 .. 8 at bursts, mean nothing -- discard trial 0 of a -z run)\n"
                 " -i beam                 observation mode: beam column `beam` of the detected stream carries the incoherent beam\n"
                 "                         (antenna powers summed over the antennas, no weights) for every consumer; 0 <= beam < N_BEAMS\n"
                 " -V file [-L corr_blocks]   observation mode: the correlator -- antenna visibilities of the analysed blocks, integrated\n"
                 "                         over corr_blocks blocks [1] per dump, to file (with -R: file.<rank>, each shard its own channels);\n"
                 "                         -j counts the 25 burn-in reads: -j 27 analyses two blocks\n"
                 " -E vis_file -G gains_file [-P]   the gain solver, no observation: every record of a -V file solved for the antenna gains\n"
                 "                         of a calibrator at the phase centre (StEFCal on the device; -P: both polarisations jointly,\n"
                 "                         one layer) and written as one record of gains_file; works on a shard's vis_file.<rank> too\n"
                 " -A gains_file           DEBUG run and observation mode: layer 0 of the last record of gains_file calibrates the\n"
                 "                         steering weights (conj(g) / |g|); its NANT / NFREQ / FIRST_CHANNEL must be the run's\n"
                 " -Y file [-J sk_blocks]  observation mode: the voltage moments -- sum |v|^2 and sum |v|^4 per (channel, polarisation,\n"
                 "                         antenna) of the analysed blocks, integrated over sk_blocks blocks [1] per dump, to file (with -R:\n"
                 "                         file.<rank>, each shard its own channels)\n"
                 " -e moments_file -O ant_file [-q chan_file] [-t n_sigma] [-m centre]   select mode, no device: the records of a -Y file\n"
                 "                         summed, the spectral-kurtosis rule applied (centre [1] +- n_sigma [5] * 2 / sqrt(columns)); flagged\n"
                 "                         antennas to ant_file, flagged channels to chan_file, one index per line (chan_file can be given to -F)\n"
                 " -f ant_file             with -E: the solver leaves the listed antennas out (gains exactly 0); with -A: they get zero weights\n"
                 " -x file -b b0,b1,... [-l n_int]   observation mode: full-Stokes follow-up beams -- I, Q, U, V (exact int64) of up to 16\n"
                 "                         of the beams per window of n_int voltage samples [N_AVERAGING; 1 = full time resolution; must\n"
                 "                         divide N_OUTPUTS_PER_GEMM * N_AVERAGING], one record per launch, to file (with -R: file.<rank>)\n"
                 " -E vis_file -Z null_file [-y n_null[:min_ratio]]   the spatial null, no observation: the dominant eigenvectors of\n"
                 "                         every record of a -V file (power iteration on the device; up to n_null [1] of 1 .. 4 per channel,\n"
                 "                         each used only if it stands min_ratio [4] above the mean of the rest) as one record of null_file;\n"
                 "                         -G may be given too; -f leaves antennas out; with -R world -r rank: vis_file.<rank> -> null_file.<rank>\n"
                 " -Z null_file            DEBUG run and observation mode: the vectors of the last record of null_file are projected out of\n"
                 "                         the steering weights (after -A's gains; -x follows the same weights; -f zeroes antennas); its\n"
                 "                         NANT / NFREQ / FIRST_CHANNEL must be the run's; with -R: null_file.<rank>\n"
                 " --events FILE [--event-tol T[,D]] [--event-veto MAXBEAMS[:IB_RATIO]]   with -S: the candidates grouped into events,\n"
                 "                         friends of friends within T samples [0] and D trials [1]; one line per event to FILE (t_start dm beam\n"
                 "                         width snr peak n_members n_beams dm_lo dm_hi t_lo t_hi snr_ib flags; with -X: FILE.<rank>); flags: 1 only\n"
                 "                         the -i column saw it, 2 more than MAXBEAMS [4] beams, 4 the -i column's S/N >= IB_RATIO [0.5] x the best\n"
                 " --stamps FILE [--stamp-shape BINS[:TBIN[:FBIN]]] [--stamp-flagged]   with --events: the dedispersed dynamic spectrum of\n"
                 "                         each unflagged event's best beam (--stamp-flagged: of flagged ones too), BINS [64] bins of TBIN samples\n"
                 "                         [0: half the width] x channels in groups of FBIN [1, must divide the band], cut from the DM stage's ring\n"
                 "                         --events without -S, --stamps without --events, the others without their parent, or malformed\n"
                 "                         numbers: beam exits with a usage error\n"
                 " --voltages FILE [--voltage-units N] [--voltage-history UNITS] [--voltage-flagged]   with --events: the dedispersed packed\n"
                 "                         voltages under each unflagged event (--voltage-flagged: under flagged ones too), N [2] gemm-units in the\n"
                 "                         input layout centred on the best member, cut from a history of UNITS gemm-units [what the search needs]\n"
                 "                         kept on the device; not with -R; --voltages without --events, the others without --voltages, or a\n"
                 "                         number < 1: beam exits with a usage error\n"
                 " --coherent V_FILE --coherent-out FILE -M dm_max [-N n_dm] [-T tsamp_ms] [--coherent-fft N] [--coherent-int n]\n"
                 "                         [--coherent-sideband +1|-1] [-A gains]   no observation: every cut of V_FILE (written with --voltages by a run\n"
                 "                         with the same -M -N -T -g -p -d -A) coherently dedispersed at the DM of its trial, for its beam alone: the beam\n"
                 "                         voltages, then overlap-save segments of N samples [the smallest power of two >= 256 whose quarter holds the\n"
                 "                         dispersion sweep across a channel; 64 .. 4096 if given] through a chirp filter, then Stokes I, Q, U, V summed\n"
                 "                         over n [1] samples, float32 [time][channel][4] per cut to FILE; a cut whose sweep needs more than 4096 samples\n"
                 "                         or that is shorter than one segment is left out and counted; with -j / -k / -E, without --coherent-out or\n"
                 "                         -M, the others without --coherent, or an N that is no power of two in range: a usage error\n"
                 " --fold F0[:F1[:PHASE0]] [--fold-dm DM] [--fold-bins N] [--fold-rows ROWS] [--fold-out FILE]   with -M: the detected stream of\n"
                 "                         every beam folded at spin frequency F0 Hz, derivative F1 Hz/s [0] and phase PHASE0 turns [0] at the first row,\n"
                 "                         dedispersed at DM pc/cc [0] (the k-th --fold-dm belongs to the k-th --fold; up to 4 --fold), into N [64] phase\n"
                 "                         bins (2 .. 4096); a dump to FILE whenever ROWS [one block's] rows or more have been folded (with -X: FILE.<rank>);\n"
                 "                         --fold without -M, the others without --fold, more than 4 --fold or malformed numbers: a usage error\n"
                 " --inject T0:DM:BEAM:FLUENCE[:SIGMA[:W]] [--inject-train F0:DM:BEAM:AMP[:DUTY[:BINS]]] [--inject-out FILE]   with -M: synthetic pulses\n"
                 "                         added to the detected rows in front of the DM stage (and of -n): a burst whose window of W rows [the smallest\n"
                 "                         power of two >= 8 SIGMA] starts at row T0 in the highest channel, dispersed at DM pc/cc, a Gaussian of SIGMA [1] rows\n"
                 "                         of FLUENCE per channel in beam BEAM (any number of --inject); a pulse train at spin frequency F0 Hz, a boxcar of\n"
                 "                         max(1, round(DUTY BINS)) of BINS [64] phase bins (DUTY [0.05]) of height AMP (up to 4 --inject-train); one line of\n"
                 "                         truth per pulse to FILE (id kind t0|f0 dm trial beam ...; with -X: FILE.<rank>); an injection option without -M,\n"
                 "                         --inject-out without a pulse, more than 4 trains or malformed numbers: a usage error\n"
                 " --ffa P_LO:P_HI [--ffa-seg N] [--ffa-dec N] [--ffa-oct N] [--ffa-widths K] [--ffa-snr SNR] [--ffa-out FILE] [--ffa-detrend BLK:WIN]\n"
                 "                         with -M: a blind periodicity search (Fast Folding Algorithm) of every DM trial and beam: the chunks decimated by --ffa-dec [1],\n"
                 "                         cut into segments of --ffa-seg [1024] samples, folded at the base periods P_LO <= p < P_HI (8 .. 512 samples)\n"
                 "                         of --ffa-oct [1] octaves, boxcar widths 1 .. 2^(K-1) [K = 3]; one line per candidate at S/N >= SNR [8] to FILE\n"
                 "                         (with -X: FILE.<rank>, trials numbered over the whole ladder); --ffa without -M, the others without --ffa or\n"
                 "                         malformed numbers: a usage error.  --ffa-detrend BLK:WIN removes red noise from every segment in\n"
                 "                         front of the fold: a running median over WIN (odd, 1 .. 129) means of BLK (a power of two, 1 .. 256, dividing\n"
                 "                         --ffa-seg) decimated samples, interpolated between the block centres; the file's header then says detrend=BLK:WIN\n"
                 " -H                      this text\n";
}

// ---------------------------------------------------------------------------------------------------------------------------------
// parse: the command line into `o`.  -1: go on; otherwise the exit status (-h, -H, an unknown option).  The long options mark a
// malformed number in their group and leave the refusal to check(); the short ones keep the reference's atoi / atof.
// ---------------------------------------------------------------------------------------------------------------------------------
int parse(int argc, char* argv[], options& o)
{
    enum { kEvents = 1000, kEventTol, kEventVeto, kStamps, kStampShape, kStampFlagged, kFold, kFoldDm, kFoldBins, kFoldRows, kFoldOut, kFfa, kFfaSeg, kFfaDec, kFfaOct, kFfaWidths, kFfaSnr, kFfaOut, kFfaDetrend, kInject, kInjectTrain, kInjectOut, kVoltages, kVoltageUnits, kVoltageHistory, kVoltageFlagged, kCoherent, kCoherentOut, kCoherentFft, kCoherentInt, kCoherentSideband, kFaraday, kFaradayOut, kFaradayPhi, kFaradayWindow };
    static const option long_options[] = {{"events", required_argument, nullptr, kEvents},       {"event-tol", required_argument, nullptr, kEventTol},
                                          {"event-veto", required_argument, nullptr, kEventVeto}, {"stamps", required_argument, nullptr, kStamps},
                                          {"stamp-shape", required_argument, nullptr, kStampShape}, {"stamp-flagged", no_argument, nullptr, kStampFlagged},
                                          {"fold", required_argument, nullptr, kFold},           {"fold-dm", required_argument, nullptr, kFoldDm},
                                          {"fold-bins", required_argument, nullptr, kFoldBins},   {"fold-rows", required_argument, nullptr, kFoldRows},
                                          {"fold-out", required_argument, nullptr, kFoldOut},
                                          {"ffa", required_argument, nullptr, kFfa},             {"ffa-seg", required_argument, nullptr, kFfaSeg},
                                          {"ffa-dec", required_argument, nullptr, kFfaDec},       {"ffa-oct", required_argument, nullptr, kFfaOct},
                                          {"ffa-widths", required_argument, nullptr, kFfaWidths}, {"ffa-snr", required_argument, nullptr, kFfaSnr},
                                          {"ffa-out", required_argument, nullptr, kFfaOut},       {"ffa-detrend", required_argument, nullptr, kFfaDetrend},
                                          {"inject", required_argument, nullptr, kInject},       {"inject-train", required_argument, nullptr, kInjectTrain},
                                          {"inject-out", required_argument, nullptr, kInjectOut},
                                          {"voltages", required_argument, nullptr, kVoltages},   {"voltage-units", required_argument, nullptr, kVoltageUnits},
                                          {"voltage-history", required_argument, nullptr, kVoltageHistory}, {"voltage-flagged", no_argument, nullptr, kVoltageFlagged},
                                          {"coherent", required_argument, nullptr, kCoherent},   {"coherent-out", required_argument, nullptr, kCoherentOut},
                                          {"coherent-fft", required_argument, nullptr, kCoherentFft}, {"coherent-int", required_argument, nullptr, kCoherentInt},
                                          {"coherent-sideband", required_argument, nullptr, kCoherentSideband},
                                          {"faraday", required_argument, nullptr, kFaraday},     {"faraday-out", required_argument, nullptr, kFaradayOut},
                                          {"faraday-phi", required_argument, nullptr, kFaradayPhi}, {"faraday-window", required_argument, nullptr, kFaradayWindow},
                                          {nullptr, 0, nullptr, 0}};
    const char* end = nullptr;
    int arg = 0;
    while ((arg = getopt_long(argc, argv, "s:g:p:d:o:D:a:c:k:K:j:w:R:r:I:M:N:T:W:Q:S:B:C:i:V:L:E:G:A:n:U:F:Y:J:e:O:q:t:m:f:x:b:l:Z:y:zPXuvhH", long_options, nullptr)) != -1) {  // src/beamformer.cu:41-43 (+ -o -D -a -v)
        switch (arg) {
            case kFold: {   // f0[:f1[:phase0]]
                fold_spec fs;
                double v[3] = {0.0, 0.0, 0.0};
                if (reals(optarg, 3, /*finite=*/false, v) < 0) o.fold.bad = true;
                fs.f0 = v[0], fs.f1 = v[1], fs.phase0 = v[2];
                o.fold.pulsars.push_back(fs);
                break;
            }
            case kFoldDm: {
                double dm = 0.0;
                if (!real(optarg, &dm) || !(dm >= 0.0)) o.fold.bad = true;
                o.fold.dms.push_back(dm);
                o.fold.given = true;
                break;
            }
            case kFoldBins:
            case kFoldRows: {
                int* field[1] = {arg == kFoldBins ? &o.fold.bins : &o.fold.rows};
                if (counts(optarg, 0, 1, field) < 0) o.fold.bad = true;
                o.fold.given = true;
                break;
            }
            case kFoldOut: o.fold.path = optarg; o.fold.given = true; break;
            case kInject:
            case kInjectTrain: {   // four to six numbers between colons
                inject_spec sp;
                sp.n = std::max(0, reals(optarg, 6, /*finite=*/true, sp.v));
                if (sp.n < 4 || !complete_pulse(sp, arg == kInjectTrain)) o.inj.bad = true;
                (arg == kInject ? o.inj.bursts : o.inj.trains).push_back(sp);
                break;
            }
            case kInjectOut: o.inj.path = optarg; break;
            case kFfa:          // p_lo:p_hi
            case kFfaDetrend: { // blk:win
                int* field[2] = {arg == kFfa ? &o.ffa.p_lo : &o.ffa.detrend_blk, arg == kFfa ? &o.ffa.p_hi : &o.ffa.detrend_win};
                if (counts(optarg, ':', 2, field) != 2) o.ffa.bad = true;
                (arg == kFfa ? o.ffa.on : o.ffa.given) = true;
                break;
            }
            case kFfaSeg:
            case kFfaDec:
            case kFfaOct:
            case kFfaWidths: {
                int* field[1] = {arg == kFfaSeg ? &o.ffa.seg : arg == kFfaDec ? &o.ffa.dec : arg == kFfaOct ? &o.ffa.oct : &o.ffa.widths};
                if (counts(optarg, 0, 1, field) < 0) o.ffa.bad = true;
                o.ffa.given = true;
                break;
            }
            case kFfaSnr:
                if (!real(optarg, &o.ffa.snr) || !(o.ffa.snr == o.ffa.snr)) o.ffa.bad = true;
                o.ffa.given = true;
                break;
            case kFfaOut: o.ffa.path = optarg; o.ffa.given = true; break;
            case kEvents: o.evt.path = optarg; break;
            case kEventTol: {   // T[,D]
                int* field[2] = {&o.evt.opt.t_tol, &o.evt.opt.dm_tol};
                if (counts(optarg, ',', 2, field) < 0) o.evt.bad = true;
                o.evt.given = true;
                break;
            }
            case kEventVeto:   // MAXBEAMS[:IB_RATIO]
                if (!whole(optarg, 0, 1000000000L, "-+ ", &o.evt.opt.max_beams, &end) ||
                    (*end == ':' ? !real(end + 1, &o.evt.opt.ib_ratio) || !(o.evt.opt.ib_ratio >= 0.0) : *end != 0))
                    o.evt.bad = true;
                o.evt.given = true;
                break;
            case kStamps: o.evt.stamps_path = optarg; break;
            case kStampShape: {   // BINS[:TBIN[:FBIN]]
                int* field[3] = {&o.evt.stamp_bins, &o.evt.stamp_tbin, &o.evt.stamp_fbin};
                if (counts(optarg, ':', 3, field) < 0 || o.evt.stamp_bins < 1 || o.evt.stamp_fbin < 1) o.evt.bad = true;
                o.evt.shape_given = true;
                break;
            }
            case kStampFlagged: o.evt.stamp_flagged = true; break;
            case kVoltages: o.vcut.path = optarg; break;
            case kVoltageUnits:
            case kVoltageHistory:   // a whole number >= 1
                if (!whole(optarg, 1, 1000000000L, "+ ", arg == kVoltageUnits ? &o.vcut.units : &o.vcut.history, &end) || *end) o.vcut.bad = true;
                o.vcut.given = true;
                break;
            case kVoltageFlagged: o.vcut.flagged = o.vcut.given = true; break;
            case kCoherent: o.coherent.path = optarg; break;
            case kCoherentOut: o.coherent.out = optarg; break;
            case kCoherentFft:
            case kCoherentInt:
            case kCoherentSideband:   // a whole number, negative ones too
                if (!whole(optarg, -1000000000L, 1000000000L, " ", arg == kCoherentFft ? &o.coherent.fft : arg == kCoherentInt ? &o.coherent.n_int : &o.coherent.sideband, &end) || *end)
                    o.coherent.bad = true;
                o.coherent.given = true;
                break;
            case kFaraday: o.faraday.path = optarg; break;
            case kFaradayOut: o.faraday.out = optarg; break;
            case kFaradayPhi: {   // lo:hi:n, n a whole number
                double v[3] = {0.0, 0.0, 0.0};
                if (reals(optarg, 3, /*finite=*/true, v) != 3 || v[2] != std::floor(v[2]) || std::fabs(v[2]) > 1e9) o.faraday.bad = true;
                o.faraday.phi_lo = v[0], o.faraday.phi_hi = v[1], o.faraday.n_phi = o.faraday.bad ? 0 : (int)v[2];
                o.faraday.given = o.faraday.phi_given = true;
                break;
            }
            case kFaradayWindow:
                if (!whole(optarg, -1000000000L, 1000000000L, "+ ", &o.faraday.window, &end) || *end) o.faraday.bad = true;
                if (!o.faraday.bad && o.faraday.window < 1) o.faraday.window = -1;
                o.faraday.given = true;
                break;
            case 's': o.sources = optarg; break;                 // :77-89
            case 'g': o.run.gpu = atoi(optarg); break;           // :92-100
            case 'p': o.positions = optarg; break;               // :102-111
            case 'd': o.directions = optarg; break;              // :113-121
            case 'o': o.output = optarg; break;
            case 'D': o.run.device = atoi(optarg); break;
            case 'a': o.cfg.n_avg = atoi(optarg); break;
            case 'j': o.junk_blocks = atol(optarg); break;
            case 'w': o.detected_path = optarg; break;
            case 'K': o.out_ring = optarg; break;
            case 'R': o.shard.world = atoi(optarg); break;
            case 'r': o.shard.rank = atoi(optarg); break;
            case 'I': o.shard.id_file = optarg; break;
            case 'M': o.dm.max = atof(optarg); break;
            case 'N': o.dm.cap = atoi(optarg); break;
            case 'T': o.dm.tsamp_ms = atof(optarg); break;
            case 'W': o.dm.path = optarg; break;
            case 'X': o.dm.split = true; break;
            case 'Q': o.dm.ring = optarg; break;
            case 'S': o.sps.snr = atof(optarg); o.sps.on = true; break;
            case 'B': o.sps.widths = atoi(optarg); o.sps.widths_given = true; break;
            case 'C': o.sps.cand_path = optarg; break;
            case 'n': o.cond.pushes = atoi(optarg); o.cond.given = true; break;
            case 'z': o.cond.zero_dm = true; break;
            case 'U': o.cond.auto_threshold = atof(optarg); o.cond.auto_given = true; break;
            case 'F': o.cond.mask_path = optarg; break;
            case 'i': o.ib.beam = atoi(optarg); o.ib.given = true; break;
            case 'V': o.corr.path = optarg; break;
            case 'L': o.corr.blocks = atoi(optarg); o.corr.blocks_given = true; break;
            case 'E': o.solve.vis = optarg; break;
            case 'G': o.solve.gains_path = optarg; break;
            case 'A': o.solve.apply = optarg; break;
            case 'P': o.solve.joint = true; break;
            case 'f': o.solve.ant_flags_path = optarg; break;
            case 'Y': o.sk.path = optarg; break;
            case 'J': o.sk.blocks = atoi(optarg); o.sk.blocks_given = true; break;
            case 'e': o.select.path = optarg; break;
            case 'O': o.select.ant_path = optarg; break;
            case 'q': o.select.chan_path = optarg; break;
            case 't': o.select.opt.n_sigma = atof(optarg); o.select.given = true; break;
            case 'm': o.select.opt.centre = atof(optarg); o.select.given = true; break;
            case 'Z': o.null.path = optarg; break;
            case 'y': {   // n_null[:min_ratio]: 1 .. BF_NULL_MAX, and a ratio >= 0 (the last -y counts)
                o.null.spec = optarg;
                bf_null_default_options(&o.null.opt);
                double ratio = o.null.opt.min_ratio;
                int n = 0;
                o.null.bad = !whole(optarg, 1, BF_NULL_MAX, "", &n, &end) || (*end == ':' ? !real(end + 1, &ratio) || !(ratio >= 0.0) : *end != 0);
                if (!o.null.bad) o.null.opt.n_null = n, o.null.opt.min_ratio = ratio;
                break;
            }
            case 'x': o.stokes.path = optarg; break;
            case 'b': o.stokes.list = optarg; break;
            case 'l': o.stokes.n_int = atoi(optarg); o.stokes.int_given = true; break;
            case 'u': o.per_unit = true; break;                   // the reference's launch pattern: one launch per gemm-unit
            case 'v': o.run.verbose = true; o.cfg.verbose = 1; break;
            case 'c': o.core = atoi(optarg); break;              // :59-65
            case 'k': o.ring_key = optarg; break;                // :66-75 (a shared-memory ring name instead of a hex key)
            case 'h': usage(true, std::cout); return EXIT_SUCCESS;  // :123-125
            case 'H': extended_usage(); return EXIT_SUCCESS;
            default: usage(true, std::cerr); return EXIT_FAILURE;
        }
    }
    return -1;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// What is read from files before any device is touched
// ---------------------------------------------------------------------------------------------------------------------------------
struct inputs {
    std::vector<uint8_t> cond_mask;          // -F, against the production band
    std::string solve_vis, null_path;        // -E / -Z as opened: with -R the null's files carry the rank, as -V's do
    std::vector<uint8_t> ant_flags;          // -f, against NANT of the vis file (-E), of the voltage file (--coherent) or of the run (-A, -Z)
    std::vector<double> gains;               // -A: layer 0 of the last record
    null_vectors nulls;                      // -Z without -E: the last record
    bool have_nulls = false;
    voltage_file_header coherent_header;     // --coherent: the geometry is the file's

    const double* gains_or_null() const { return gains.empty() ? nullptr : gains.data(); }
    const null_vectors* nulls_or_null() const { return have_nulls ? &nulls : nullptr; }
    const uint8_t* flags_or_null() const { return ant_flags.empty() ? nullptr : ant_flags.data(); }
    // a run's weights take the flags only where gains or nulls condition them
    const uint8_t* weight_flags() const { return gains.empty() && !have_nulls ? nullptr : flags_or_null(); }
};

// -F: channel indices to mask, one per line, # comments (its messages are its own: they name a channel index, read_index_file an index)
int read_channel_mask(const std::string& path, std::vector<uint8_t>* mask)
{
    const int n_freq = production_band().n_freq;
    std::ifstream in(path);
    if (!in) return refuse("-F %s: could not be read", path.c_str());
    mask->assign((size_t)n_freq, 0);
    std::string line;
    while (std::getline(in, line)) {
        line = line.substr(0, line.find('#'));
        const size_t a = line.find_first_not_of(" \t\r");
        if (a == std::string::npos) continue;
        char* end = nullptr;
        const long ch = strtol(line.c_str() + a, &end, 10);
        while (*end == ' ' || *end == '\t' || *end == '\r') end++;
        if (end == line.c_str() + a || *end || ch < 0 || ch >= n_freq) return refuse("-F %s: '%s' is not a channel index 0 .. %d", path.c_str(), line.c_str() + a, n_freq - 1);
        (*mask)[(size_t)ch] = 1;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// check: the parent / child and range rules, in the order in which a command line with several faults reports them.  0, or the exit
// status of the first refusal.  Two things that are not rules sit among them because their refusals rank there: the -F file is read
// between -U's rule and -i's, and -b's list is parsed into o.stokes.beams.
// ---------------------------------------------------------------------------------------------------------------------------------
int check(options& o, inputs* in)
{
    const bf_config& band = production_band();
    if (o.sps.on && !o.dm.on()) return refuse("-S (single-pulse search) requires the DM stage: give -M dm_max");
    if (!o.sps.on && (o.sps.widths_given || !o.sps.cand_path.empty())) return refuse("-B / -C belong to the single-pulse search: give -S snr (and -M dm_max)");
    if (!o.fold.pulsars.empty() && !o.dm.on()) return refuse("--fold (pulsar folding) requires the DM stage: give -M dm_max");
    if (o.fold.pulsars.empty() && o.fold.given) return refuse("--fold-dm / --fold-bins / --fold-rows / --fold-out belong to the pulsar folder: give --fold F0[:F1[:PHASE0]]");
    if (o.fold.bad || o.fold.pulsars.size() > (size_t)BF_PSR_MAX_PULSARS || o.fold.dms.size() > o.fold.pulsars.size() ||
        (!o.fold.pulsars.empty() && (o.fold.bins < 2 || o.fold.bins > BF_PSR_MAX_BINS || o.fold.rows < 0)))
        return refuse("--fold F0[:F1[:PHASE0]] (at most %d), --fold-dm DM >= 0 (one per --fold at most), --fold-bins 2 .. %d, --fold-rows ROWS: "
                      "malformed, too many or out of range", BF_PSR_MAX_PULSARS, BF_PSR_MAX_BINS);
    if ((o.inj.on() || !o.inj.path.empty()) && !o.dm.on()) return refuse("--inject / --inject-train / --inject-out (pulse injection) require the DM stage: give -M dm_max");
    if (!o.inj.on() && !o.inj.path.empty()) return refuse("--inject-out belongs to the pulse injection: give --inject T0:DM:BEAM:FLUENCE or --inject-train F0:DM:BEAM:AMP");
    if (o.inj.bad || o.inj.trains.size() > (size_t)BF_INJ_MAX_TRAINS || o.inj.bursts.size() + o.inj.trains.size() > (size_t)BF_INJ_MAX_PULSES)
        return refuse("--inject T0:DM:BEAM:FLUENCE[:SIGMA[:W]], --inject-train F0:DM:BEAM:AMP[:DUTY[:BINS]] (at most %d): malformed, too many or out of range", BF_INJ_MAX_TRAINS);
    if (o.ffa.on && !o.dm.on()) return refuse("--ffa (periodicity search) requires the DM stage: give -M dm_max");
    if (!o.ffa.on && o.ffa.given)
        return refuse("--ffa-seg / --ffa-dec / --ffa-oct / --ffa-widths / --ffa-snr / --ffa-out / --ffa-detrend belong to the periodicity search: give --ffa P_LO:P_HI");
    if (o.ffa.bad) return refuse("--ffa P_LO:P_HI, --ffa-seg N, --ffa-dec N, --ffa-oct N, --ffa-widths N, --ffa-snr SNR, --ffa-detrend BLK:WIN: malformed number");
    if (o.evt.bad) return refuse("--event-tol T[,D], --event-veto MAXBEAMS[:IB_RATIO], --stamp-shape BINS[:TBIN[:FBIN]]: malformed or negative number");
    if (!o.evt.path.empty() && !o.sps.on) return refuse("--events groups the candidates of the single-pulse search: give -S snr (and -M dm_max)");
    if (o.evt.path.empty() && (o.evt.given || !o.evt.stamps_path.empty())) return refuse("--event-tol / --event-veto / --stamps belong to the event builder: give --events FILE");
    if (o.evt.stamps_path.empty() && (o.evt.shape_given || o.evt.stamp_flagged)) return refuse("--stamp-shape / --stamp-flagged belong to the stamps: give --stamps FILE");
    if (o.vcut.bad) return refuse("--voltage-units N, --voltage-history UNITS: need a whole number >= 1");
    if (o.vcut.path.empty() && o.vcut.given) return refuse("--voltage-units / --voltage-history / --voltage-flagged belong to the voltage cuts: give --voltages FILE");
    if (!o.vcut.path.empty() && o.evt.path.empty()) return refuse("--voltages cuts the voltages of the event builder's events: give --events FILE");
    if (!o.vcut.path.empty() && o.shard.world > 1)
        return refuse("--voltages is not available in a sharded run (-R): a trigger is not sent to the ranks that hold the other channels");
    if (o.coherent.path.empty() && (!o.coherent.out.empty() || o.coherent.given))
        return refuse("--coherent-out / --coherent-fft / --coherent-int / --coherent-sideband belong to coherent dedispersion: give --coherent V_FILE");
    if (!o.coherent.path.empty()) {
        if (o.observe() || !o.solve.vis.empty()) return refuse("--coherent runs no observation and no solver: leave out -j / -k / -E");
        if (o.coherent.out.empty()) return refuse("--coherent needs --coherent-out FILE (where the Stokes parameters go)");
        if (!o.dm.on()) return refuse("--coherent takes the DM of a cut from the ladder of the run that wrote it: give that run's -M dm_max (and -N, -T)");
        bool pow2 = false;
        for (int n = 64; n <= 4096; n *= 2) pow2 = pow2 || o.coherent.fft == n;
        if (o.coherent.bad || (o.coherent.fft != 0 && !pow2) || o.coherent.n_int < 1 || (o.coherent.sideband != 1 && o.coherent.sideband != -1))
            return refuse("--coherent-fft N: a power of two 64 .. 4096; --coherent-int n: a whole number >= 1; --coherent-sideband: +1 or -1");
        if (!(o.dm.tsamp_ms > 0.0)) return refuse("-T %g: the sample time must be positive", o.dm.tsamp_ms);
    }
    // (the mode's refusals end in its synopsis: the texts of -h and -H are recorded byte for byte and do not list it)
    static const char* const synopsis = "usage: beam --faraday C_FILE --faraday-out FILE [--faraday-phi LO:HI:N] [--faraday-window ROWS] [-F mask_file] [-g gpu] [-D device]";
    if (o.faraday.path.empty() && (!o.faraday.out.empty() || o.faraday.given))
        return refuse("--faraday-out / --faraday-phi / --faraday-window belong to Faraday synthesis: give --faraday C_FILE\n      %s", synopsis);
    if (!o.faraday.path.empty()) {
        if (o.observe() || !o.solve.vis.empty() || !o.coherent.path.empty())
            return refuse("--faraday runs no observation, no solver and no dedispersion: leave out -j / -k / -E / --coherent\n      %s", synopsis);
        if (o.dm.on() || o.sps.on || o.cond.given || !o.solve.apply.empty() || !o.null.path.empty())
            return refuse("--faraday takes nothing from the DM stage, the search, the conditioner or the weights: leave out -M / -S / -n / -A / -Z\n      %s", synopsis);
        if (o.faraday.out.empty()) return refuse("--faraday needs --faraday-out FILE (where the spectra and peaks go)\n      %s", synopsis);
        if (o.faraday.bad) return refuse("--faraday-phi LO:HI:N: three numbers, N whole; --faraday-window ROWS: a whole number\n      %s", synopsis);
        if (o.faraday.n_phi > 4096) return refuse("--faraday-phi: N = %d; at most 4096 depths\n      %s", o.faraday.n_phi, synopsis);
        if (o.faraday.phi_given && (o.faraday.n_phi < 1 || o.faraday.phi_hi < o.faraday.phi_lo || (o.faraday.n_phi == 1 && o.faraday.phi_hi != o.faraday.phi_lo)))
            return refuse("--faraday-phi %g:%g:%d: an empty grid; LO <= HI and N >= 1 (N = 1: LO = HI)\n      %s", o.faraday.phi_lo, o.faraday.phi_hi, o.faraday.n_phi, synopsis);
        if (o.faraday.window < 0) return refuse("--faraday-window: at least 1 row\n      %s", synopsis);
    }
    if (!o.evt.stamps_path.empty() && band.n_freq % o.evt.stamp_fbin != 0)
        return refuse("--stamp-shape: FBIN %d does not divide the band's %d channels", o.evt.stamp_fbin, band.n_freq);
    if (o.sps.on && (o.sps.widths < 1 || o.sps.widths > 8)) return refuse("-B %d: n_widths must be 1 .. 8", o.sps.widths);
    const bool cond_extra = o.cond.zero_dm || o.cond.auto_given || (!o.cond.mask_path.empty() && o.faraday.path.empty());   // (--faraday's -F is its own)
    if ((o.cond.given || cond_extra) && !o.dm.on()) return refuse("-n / -z / -U / -F (conditioner) require the DM stage: give -M dm_max");
    if (!o.cond.given && cond_extra) return refuse("-z / -U / -F belong to the conditioner: give -n baseline_pushes");
    if (o.cond.given && (o.cond.pushes < 1 || o.cond.pushes > 64)) return refuse("-n %d: baseline_pushes must be 1 .. 64", o.cond.pushes);
    if (o.cond.auto_given && !(o.cond.auto_threshold >= 0.0))
        return refuse("-U %s: the automatic mask's threshold must be >= 0", std::to_string(o.cond.auto_threshold).c_str());
    if (!o.cond.mask_path.empty())
        if (int rc = read_channel_mask(o.cond.mask_path, &in->cond_mask)) return rc;
    if (o.ib.given && (o.ib.beam < 0 || o.ib.beam >= o.cfg.n_beams)) return refuse("-i %d: the incoherent beam takes a beam index 0 .. %d", o.ib.beam, o.cfg.n_beams - 1);
    if (o.ib.given && !o.observe()) return refuse("-i (incoherent beam) belongs to the observation mode: give -j n_blocks or -k ring");
    if (o.corr.blocks_given && o.corr.path.empty()) return refuse("-L (blocks per dump) belongs to the correlator: give -V vis_file");
    if (o.corr.blocks_given && o.corr.blocks < 1) return refuse("-L %d: the correlator integrates at least one block per dump", o.corr.blocks);
    if (!o.corr.path.empty() && !o.observe()) return refuse("-V (correlator) belongs to the observation mode: give -j n_blocks or -k ring");
    if (o.sk.blocks_given && o.sk.path.empty()) return refuse("-J (blocks per dump) belongs to the voltage moments: give -Y moments_file");
    if (o.sk.blocks_given && o.sk.blocks < 1) return refuse("-J %d: the moments integrate at least one block per dump", o.sk.blocks);
    if (!o.sk.path.empty() && !o.observe()) return refuse("-Y (voltage moments) belongs to the observation mode: give -j n_blocks or -k ring");
    if (o.stokes.path.empty() && (!o.stokes.list.empty() || o.stokes.int_given)) return refuse("-b / -l belong to the Stokes beams: give -x stokes_file");
    if (!o.stokes.path.empty()) {
        if (!o.observe()) return refuse("-x (Stokes beams) belongs to the observation mode: give -j n_blocks or -k ring");
        if (o.stokes.list.empty()) return refuse("-x needs -b b0,b1,... (the beams to follow)");
        std::string why;
        if (!parse_beam_list(o.stokes.list.c_str(), band.n_beams, &o.stokes.beams, &why)) return refuse("-b %s", why.c_str());
        const int samples = band.n_out_per_gemm * band.n_avg;
        if (o.stokes.int_given && (o.stokes.n_int < 1 || samples % o.stokes.n_int))
            return refuse("-l %d: the window must be at least 1 and divide the %d samples of a gemm-unit", o.stokes.n_int, samples);
    }
    if (o.select.path.empty() && (!o.select.ant_path.empty() || !o.select.chan_path.empty() || o.select.given))
        return refuse("-O / -q / -t / -m belong to the select mode: give -e moments_file");
    if (!o.solve.ant_flags_path.empty() && o.solve.vis.empty() && o.solve.apply.empty() && o.null.path.empty())
        return refuse("-f (antenna flags) belongs to the solvers or to conditioned weights: give -E vis_file, -A gains_file or -Z null_file");
    if (!o.select.path.empty()) {   // select mode runs nothing else, and the solvers' rules below never see its command line
        if (o.observe() || !o.solve.vis.empty() || !o.solve.apply.empty() || !o.null.path.empty())
            return refuse("-e (select flags) runs nothing else: leave out -j / -k / -E / -A / -Z");
        if (o.select.ant_path.empty()) return refuse("-e needs -O ant_file (where the antenna flags go)");
        return 0;
    }
    if (!o.solve.gains_path.empty() && o.solve.vis.empty()) return refuse("-G (where the gains go) belongs to the gain solver: give -E vis_file");
    if (o.solve.joint && o.solve.vis.empty()) return refuse("-P (joint polarisations) belongs to the gain solver: give -E vis_file -G gains_file");
    if (!o.null.spec.empty()) {
        if (o.solve.vis.empty() || o.null.path.empty()) return refuse("-y (vectors per channel) belongs to the spatial null's solve mode: give -E vis_file -Z null_file");
        if (o.null.bad) return refuse("-y %s: n_null must be 1 .. %d and min_ratio, if given, a number >= 0", o.null.spec.c_str(), BF_NULL_MAX);
    }
    if (!o.solve.vis.empty()) {   // solve mode: no observation of either kind
        if (o.observe()) return refuse("-E (gain solver) runs no observation: leave out -j / -k");
        if (o.solve.gains_path.empty() && o.null.path.empty())
            return refuse("-E needs -G gains_file (where the gains go) or -Z null_file (where the interferer vectors go)");
        if (!o.solve.apply.empty()) return refuse("-A (apply gains) belongs to a run; -E only solves");
    }
    return 0;
}

// -f, once, against `n_ant` antennas
int load_ant_flags(const options& o, int n_ant, inputs* in)
{
    std::string why;
    if (o.solve.ant_flags_path.empty() || !in->ant_flags.empty() || read_index_file(o.solve.ant_flags_path.c_str(), n_ant, &in->ant_flags, &why)) return 0;
    return refuse("-f %s", why.c_str());
}

std::string with_rank(const std::string& path, int rank) { return path + "." + std::to_string(rank); }

// ---------------------------------------------------------------------------------------------------------------------------------
// load: the files a mode reads before any device is touched -- the headers of -E and --coherent, -A's gains, -Z's vectors, -f's flags.
// A DEBUG run has the DEBUG geometry, observation mode a rank's share of the production band.
// ---------------------------------------------------------------------------------------------------------------------------------
int load(const options& o, inputs* in)
{
    const int world = o.shard.world, rank = o.shard.rank;
    const bool sharded_files = world > 1 && rank >= 0 && rank < world;
    const bool solve = !o.solve.vis.empty(), coherent = !o.coherent.path.empty(), observe = o.observe();
    in->solve_vis = solve && !o.null.path.empty() && sharded_files ? with_rank(o.solve.vis, rank) : o.solve.vis;
    in->null_path = !o.null.path.empty() && sharded_files && (solve || observe) ? with_rank(o.null.path, rank) : o.null.path;
    // this rank's share of the band, as -A and -Z find it in their headers
    const bf_config& run_cfg = observe ? production_band() : o.cfg;
    const int n_ant = run_cfg.n_ant;
    const int n_freq = observe && world >= 1 && run_cfg.n_freq % world == 0 ? run_cfg.n_freq / world : run_cfg.n_freq;
    const int first = observe && rank >= 0 ? rank * n_freq : 0;
    std::string why;
    if (solve) {
        record_file_header vh;
        if (!read_record_file_header(in->solve_vis.c_str(), &vh, &why) || vh.content != "visibilities")
            return refuse("-E %s", why.empty() ? (in->solve_vis + " is not a file of visibilities").c_str() : why.c_str());
        if (int rc = load_ant_flags(o, vh.n_ant, in)) return rc;
    }
    if (coherent) {
        voltage_file_header& vh = in->coherent_header;
        if (!read_voltage_header(o.coherent.path.c_str(), &vh, &why)) return refuse("--coherent %s", why.c_str());
        if (!o.solve.apply.empty() && !read_gains_layer(o.solve.apply.c_str(), vh.n_ant, vh.n_freq, vh.first_channel, &in->gains, &why)) return refuse("-A %s", why.c_str());
        if (int rc = load_ant_flags(o, vh.n_ant, in)) return rc;
    }
    if (coherent_file_header fh; !o.faraday.path.empty() && !read_coherent_header(o.faraday.path.c_str(), &fh, &why))   // (only whether it is one: the mode reads it itself)
        return refuse("--faraday %s", why.c_str());
    if (!o.solve.apply.empty() && !coherent) {
        if (!read_gains_layer(o.solve.apply.c_str(), n_ant, n_freq, first, &in->gains, &why)) return refuse("-A %s", why.c_str());
        if (int rc = load_ant_flags(o, n_ant, in)) return rc;
    }
    if (!o.null.path.empty() && !solve) {
        if (!read_null_vectors(in->null_path.c_str(), n_ant, n_freq, first, &in->nulls, &why)) return refuse("-Z %s", why.c_str());
        in->have_nulls = true;
        if (int rc = load_ant_flags(o, n_ant, in)) return rc;
    }
    return 0;
}

// a failure of the device or of the library behind it, as the reference's gpuErrchk reports it (src/beamformer.cuh:26)
int gpu_assert(int rc)
{
    fprintf(stderr, "GPUassert: %s (%d)\n", bf_last_error(), rc);
    return EXIT_FAILURE;
}

const char* or_null(const std::string& s) { return s.empty() ? nullptr : s.c_str(); }

// -p / -d, or the built-in layout where a file is missing or unreadable
void read_layout(const options& o, int n_ant, int n_beams, std::vector<antenna>* pos, std::vector<beam_direction>* dir)
{
    pos->resize((size_t)n_ant);
    dir->resize((size_t)n_beams);
    if (o.positions.empty() || read_in_position_locations(o.positions.c_str(), n_ant, pos->data()) != 0) default_positions(n_ant, pos->data());
    if (o.directions.empty() || read_in_beam_directions(o.directions.c_str(), n_beams, dir->data()) != 0) default_directions(n_beams, dir->data());
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The modes that run no observation
// ---------------------------------------------------------------------------------------------------------------------------------

// -e: flags from a -Y file, host only
int run_select(const options& o)
{
    if (select_moments_file(o.select.path.c_str(), o.select.opt, o.select.ant_path.c_str(), or_null(o.select.chan_path), std::cout) != BF_OK)
        return refuse("-e %s", bf_last_error());
    return 0;
}

// -E / -G / -Z: the gain solver and the spatial null on a file of visibilities
int run_solve(const options& o, const inputs& in)
{
    uint64_t n_records = 0;
    if (!o.solve.gains_path.empty()) {
        int rc = solve_vis_file(in.solve_vis.c_str(), o.solve.gains_path.c_str(), o.solve.joint, o.run.device, &n_records, std::cout, in.flags_or_null());
        if (rc != BF_OK) return gpu_assert(rc);
        std::cout << "Wrote " << n_records << " gain records to " << o.solve.gains_path << std::endl;
    }
    if (!in.null_path.empty()) {
        int rc = null_vis_file(in.solve_vis.c_str(), in.null_path.c_str(), o.null.opt, o.run.device, &n_records, std::cout, in.flags_or_null());
        if (rc != BF_OK) return gpu_assert(rc);
        std::cout << "Wrote " << n_records << " null records to " << in.null_path << std::endl;
    }
    return 0;
}

// --coherent: a file of voltage cuts to coherently dedispersed Stokes parameters
int run_coherent(const options& o, const inputs& in)
{
    std::vector<antenna> pos;
    std::vector<beam_direction> dir;
    read_layout(o, in.coherent_header.n_ant, production_band().n_beams, &pos, &dir);
    coherent_options copt;
    copt.voltages_path = o.coherent.path.c_str();
    copt.out_path = o.coherent.out.c_str();
    copt.dm_max = o.dm.max;
    copt.tsamp_ms = o.dm.tsamp_ms;
    copt.n_dm_cap = o.dm.cap;
    copt.n_fft = o.coherent.fft;
    copt.n_int = o.coherent.n_int;
    copt.sideband = o.coherent.sideband;
    copt.gpu = o.run.gpu;
    copt.device = o.run.device;
    copt.pos = pos.data();
    copt.dir = dir.data();
    copt.gains = in.gains_or_null();
    copt.ant_flags = in.gains.empty() ? nullptr : in.flags_or_null();
    uint64_t n_written = 0, n_refused = 0;
    const int rc = coherent_voltage_file(copt, &n_written, &n_refused, std::cout);
    if (rc != BF_OK) return gpu_assert(rc);
    std::cout << "Wrote " << n_written << " coherently dedispersed cuts to " << o.coherent.out << std::endl;
    return 0;
}

// --faraday: a file of coherently dedispersed Stokes parameters to rotation-measure spectra, fits and peaks
int run_faraday(const options& o, const inputs& in)
{
    faraday_options fopt;
    fopt.coherent_path = o.faraday.path.c_str();
    fopt.out_path = o.faraday.out.c_str();
    fopt.n_phi = o.faraday.n_phi;
    fopt.phi_lo = o.faraday.phi_lo;
    fopt.phi_hi = o.faraday.phi_hi;
    fopt.window = o.faraday.window;
    fopt.chan_mask = in.cond_mask.empty() ? nullptr : in.cond_mask.data();
    fopt.n_mask = (int)in.cond_mask.size();
    fopt.gpu = o.run.gpu;
    fopt.device = o.run.device;
    uint64_t n_written = 0, n_left_out = 0;
    const int rc = faraday_coherent_file(fopt, &n_written, &n_left_out, std::cout);
    if (rc != BF_OK) return gpu_assert(rc);
    std::cout << "Wrote " << n_written << " Faraday records to " << o.faraday.out << std::endl;
    return 0;
}

// the reference's DEBUG run: synthetic point sources through the loop, the table of beam responses to -o
int run_debug(const options& o, const inputs& in)
{
    debug_run_options opt = o.run;
    opt.positions = or_null(o.positions);
    opt.directions = or_null(o.directions);
    opt.sources = or_null(o.sources);
    opt.output = o.output.c_str();
    opt.block_launch = !o.per_unit;
    opt.gains = in.gains_or_null();
    opt.nulls = in.nulls_or_null();
    opt.ant_flags = in.weight_flags();
    debug_run_result res;
    int rc = run_debug_observation(o.cfg, opt, &res, nullptr, std::cout);
    if (rc != BF_OK) return gpu_assert(rc);  // the reference exit()s inside gpuErrchk; the driver keeps that policy here
    std::cout << "Freeing CUDA Structures" << std::endl;
    std::cout << "Freed GPU memory" << std::endl;
    std::cout << "Freed CPU memory" << std::endl;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Observation (production) mode, -j / -k: N_AVERAGING 16.  What its steps share, then the steps in the order in which they run: each
// wires one stage into `oopt`, opens what the stage writes to, and returns 0 or the exit status of a refusal.
// ---------------------------------------------------------------------------------------------------------------------------------
struct observation {
    const options& o;
    const inputs& in;
    bf_config band;    // the whole sub-band (what the gather root's sink receives)
    bf_config shard;   // this rank's channels of it
    int rank;
    bf_comm* comm = nullptr;
    observation_options oopt;
    std::unique_ptr<block_source> src;
    // -M: ladder and delays over the WHOLE sub-band this run covers (world x n_freq channels), and this rank's trials of it
    std::vector<float> freq;        // the band's channel frequencies
    std::vector<int32_t> delays;    // [n_dm][band.n_freq]
    int n_dm = 0, my_first = 0, my_trials = 0, my_dmax = 0;
    bool dm_here = false;           // this rank runs the DM stage -- and the search, conditioner, folder, injector and ffa, which run where it runs
    std::vector<bf_psr_model> fold_models;
    std::vector<int32_t> fold_delays;
    inj_plan inj;
    // what the run writes to, and the names the closing lines print (with -X or -R they carry the rank)
    std::unique_ptr<detected_sink> sink;
    std::unique_ptr<dm_file_sink> dm_sink;
    std::unique_ptr<dm_ring_sink> dm_rsink;
    std::unique_ptr<sps_file_sink> cand_sink;
    std::unique_ptr<event_file_sink> event_sink;
    std::unique_ptr<stamp_file_sink> stamp_sink;
    std::unique_ptr<voltage_file_sink> vcut_sink;
    std::unique_ptr<psr_file_sink> fold_sink;
    std::unique_ptr<ffa_file_sink> ffa_sink;
    std::unique_ptr<vis_file_sink> vis_sink;
    std::unique_ptr<sk_file_sink> sk_sink;
    std::unique_ptr<stokes_file_sink> stokes_sink;
    std::string sink_name, dm_path, cand_path, events_path, stamps_path, ffa_path, vis_path, sk_path, stokes_path;

    observation(const options& o_, const inputs& in_) : o(o_), in(in_), band(production_band()), shard(production_band()), rank(o_.shard.rank)
    {
        band.verbose = shard.verbose = o.cfg.verbose;
    }
    int first_channel() const { return rank * shard.n_freq; }
    int rows_per_block() const { return shard.n_gemms_per_block * shard.n_out_per_gemm; }
    // a file of the DM side: one per shard where the trials are split (-X), the trials numbered over the whole ladder
    std::string per_trial_share(const std::string& path) const { return path.empty() || !oopt.dm_split_trials ? path : with_rank(path, rank); }
    // a file of the voltage side: every shard writes its own channels
    std::string per_shard(const std::string& path) const { return comm ? with_rank(path, rank) : path; }
};

template <class Sink>
bool opened(Sink& s)
{
    if constexpr (std::is_base_of<detected_sink, Sink>::value)
        return s.ok() && s.is_open();
    else
        return s.is_open();
}

// hands a new sink to its slot; one that did not open is a refusal
template <class Slot, class Sink>
int open_or_refuse(std::unique_ptr<Slot>& slot, Sink* sink, const std::string& name, const char* fmt = "could not open %s")
{
    slot.reset(sink);
    return opened(*sink) ? 0 : refuse(fmt, name.c_str());
}

// Rank 0 publishes the unique id.  A stale id (a crashed run, a reused name) would make the other ranks join a communicator that no
// longer exists and hang: rank 0 removes whatever is there, writes a fresh file it alone created (O_EXCL | O_NOFOLLOW: no symlink is
// followed) and renames it into place -- readers see nothing or the whole id.
int publish_id(const std::string& id_file, char (&id)[BF_COMM_ID_BYTES])
{
    if (bf_comm_unique_id(id) != BF_OK) {
        fprintf(stderr, "GPUassert: %s\n", bf_last_error());
        return EXIT_FAILURE;
    }
    const std::string tmp = id_file + ".tmp";
    (void)unlink(id_file.c_str());
    (void)unlink(tmp.c_str());
    const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW, 0600);
    const bool ok = fd >= 0 && write(fd, id, sizeof id) == (ssize_t)sizeof id;
    if (fd >= 0) close(fd);
    if (!ok || rename(tmp.c_str(), id_file.c_str()) != 0) {
        perror("beam: publishing the unique id");
        return EXIT_FAILURE;
    }
    return 0;
}

// the other ranks wait for it, up to 2 minutes
int await_id(const std::string& id_file, int rank, char (&id)[BF_COMM_ID_BYTES])
{
    for (int tries = 0; tries < 1200; tries++) {
        std::ifstream in(id_file, std::ios::binary);
        if (in && in.read(id, sizeof id) && in.gcount() == (std::streamsize)sizeof id) return 0;
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
    }
    return refuse("rank %d never saw the unique id in %s", rank, id_file.c_str());
}

// -R world -r rank -I idfile: this rank's shard of the band, and the communicator that gathers the shards' powers
int join_shards(observation& ob)
{
    const int world = ob.o.shard.world, rank = ob.rank;
    const std::string& id_file = ob.o.shard.id_file;
    if (world < 1 || rank < 0 || rank >= world || ob.band.n_freq % world)
        return refuse("-R %d -r %d: need 0 <= rank < world and world dividing %d channels", world, rank, ob.band.n_freq);
    ob.shard.n_freq /= world;
    if (world == 1 && id_file.empty()) return 0;
    if (id_file.empty()) return refuse("-R needs -I idfile (where rank 0 publishes the RCCL unique id)");
    char id[BF_COMM_ID_BYTES];
    if (int rc = rank == 0 ? publish_id(id_file, id) : await_id(id_file, rank, id)) return rc;
    if (bf_comm_create(rank, world, id, ob.o.run.device, &ob.comm) != BF_OK) {
        fprintf(stderr, "GPUassert: %s\n", bf_last_error());
        return EXIT_FAILURE;
    }
    std::cout << "Shard " << rank << " of " << world << ": channels " << ob.first_channel() << " .. " << ob.first_channel() + ob.shard.n_freq - 1 << std::endl;
    return 0;
}

// where the voltage blocks come from: a PSRDADA ring (-k hexkey, PSRDADA builds), the shared-memory ring (-k name) or the in-memory junk source (-j)
int open_source(observation& ob)
{
    const options& o = ob.o;
#ifdef DSABF_WITH_PSRDADA
    unsigned in_key = 0;
    char trailing = 0;
    if (!o.ring_key.empty() && sscanf(o.ring_key.c_str(), "%x%c", &in_key, &trailing) == 1) {   // -k baab: src/beamformer.cu:66-75
        char name[] = "beam";
        dada_block_source* s = new dada_block_source(name, o.core, in_key, std::cout);        // :132
        ob.src.reset(s);
        if (!s->ok()) return EXIT_FAILURE;
        s->expect_block_bytes(bf_bytes_per_block(&ob.shard));
        ob.oopt.burn_in = kBurnIn;                                                           // BURNIN reads, :348-355
        return 0;
    }
#endif
    if (!o.ring_key.empty()) {  // -k: blocks from the shared-memory ring (the PSRDADA stand-in), no burn-in reads
        shm_block_source* s = new shm_block_source(o.ring_key.c_str(), o.core, /*pin=*/true, std::cout);
        ob.src.reset(s);
        if (!s->ok()) return EXIT_FAILURE;  // "Error: could not connect to dada buffer", src/dada_handler.hh:35-38
        s->expect_block_bytes(bf_bytes_per_block(&ob.shard));
        return 0;
    }
    junk_block_source* s = new junk_block_source(ob.shard, (uint64_t)o.junk_blocks);   // -j: the in-memory dada_junkdb source
    ob.src.reset(s);
    if (!s->ok()) return refuse("could not allocate the junk ring");
    ob.oopt.burn_in = kBurnIn;
    return 0;
}

// the run's own options, and -K / -w: where the detected stream goes (only the gather root has a consumer)
int open_detected_sink(observation& ob)
{
    const options& o = ob.o;
    observation_options& oopt = ob.oopt;
    oopt.gpu = o.run.gpu;
    oopt.device = o.run.device;
    oopt.verbose = o.run.verbose;
    oopt.world = o.shard.world;
    oopt.rank = ob.rank;
    oopt.comm = ob.comm;
    oopt.incoherent_beam = o.ib.beam;
    oopt.gains = ob.in.gains_or_null();
    oopt.nulls = ob.in.nulls_or_null();
    oopt.ant_flags = ob.in.weight_flags();
    const bf_config& sink_cfg = ob.comm ? ob.band : ob.shard;
    const bool consumer = !ob.comm || ob.rank == 0;
    if (consumer && !o.out_ring.empty()) {  // -K: hand the detected stream to another process through a shared-memory ring
        ob.sink_name = "ring " + o.out_ring;
        if (int rc = open_or_refuse(ob.sink, new ring_sink(sink_cfg, o.out_ring.c_str(), 8, o.run.gpu), o.out_ring, "could not create ring %s")) return rc;
    } else if (consumer && !o.detected_path.empty()) {  // -w: keep the detected stream in a file (the reference drops it, README.md:149)
        ob.sink_name = o.detected_path;
        if (int rc = open_or_refuse(ob.sink, new file_sink(sink_cfg, o.detected_path.c_str(), o.run.gpu), o.detected_path)) return rc;
    }
    oopt.sink = ob.sink.get();
    return 0;
}

// -M: the DM stage.  Ladder and delay law of sandbox/Dispersion Theory.ipynb (cells 1-2 and 5), referred to the band's highest frequency
// (channel 0): every delay is >= 0.  -X: every rank receives the band and takes its share of the trials.  -W / -Q: where the chunks go.
int plan_dm_stage(observation& ob)
{
    const options& o = ob.o;
    observation_options& oopt = ob.oopt;
    if (!o.dm.on()) return 0;
    const int n_freq = ob.band.n_freq;
    std::vector<double> dms = dm_trials(0.0, o.dm.max);
    if (o.dm.cap > 0 && (int)dms.size() > o.dm.cap) {
        std::vector<double> pick;
        for (int i = 0; i < o.dm.cap; i++) pick.push_back(dms[(size_t)((double)i * (dms.size() - 1) / (o.dm.cap > 1 ? o.dm.cap - 1 : 1))]);
        dms.swap(pick);
    }
    ob.n_dm = (int)dms.size();
    ob.freq.resize((size_t)n_freq);
    for (int c = 0; c < n_freq; c++) ob.freq[(size_t)c] = channel_frequency_weights(o.run.gpu, c);
    ob.delays.resize((size_t)ob.n_dm * n_freq);
    dm_delays(dms.data(), ob.n_dm, ob.freq.data(), n_freq, ob.freq[0], o.dm.tsamp_ms, ob.delays.data());
    auto largest = [&](int first, int count) {
        int dmax = 0;
        for (size_t i = (size_t)first * n_freq; i < (size_t)(first + count) * n_freq; i++) dmax = ob.delays[i] > dmax ? ob.delays[i] : dmax;
        return dmax;
    };
    std::cout << "DM stage: " << ob.n_dm << " trials 0 .. " << dms.back() << " pc/cc, largest delay " << largest(0, ob.n_dm) << " samples of " << o.dm.tsamp_ms << " ms"
              << std::endl;
    oopt.dm_delays = ob.delays.data();
    oopt.n_dm = ob.n_dm;
    ob.my_trials = ob.n_dm;
    if (o.dm.split && ob.comm) {
        oopt.gather_root = BF_GATHER_ROOT_ALL;
        oopt.dm_split_trials = true;
        dm_trial_share(ob.n_dm, o.shard.world, ob.rank, &ob.my_first, &ob.my_trials);
        if (ob.my_trials > 0)
            std::cout << "Shard " << ob.rank << " dedisperses trials " << ob.my_first << " .. " << ob.my_first + ob.my_trials - 1 << std::endl;
        else   // (more shards than trials: this one beamforms and sends its channels, and runs no DM-side stage)
            std::cout << "Shard " << ob.rank << " dedisperses no trials: the ladder has " << ob.n_dm << ", fewer than the " << o.shard.world << " shards" << std::endl;
    }
    ob.my_dmax = largest(ob.my_first, ob.my_trials);
    ob.dm_here = ob.my_trials > 0 && (!ob.comm || ob.rank == 0 || oopt.dm_split_trials);
    ob.dm_path = ob.per_trial_share(o.dm.path);
    if (!ob.dm_path.empty() && ob.dm_here) {
        if (int rc = open_or_refuse(ob.dm_sink, new dm_file_sink(ob.shard, n_freq, ob.my_trials, ob.my_dmax, ob.dm_path.c_str(), o.run.gpu, ob.my_first), ob.dm_path)) return rc;
        oopt.dm_sink = ob.dm_sink.get();
    } else if (!o.dm.ring.empty() && ob.dm_here) {   // -Q: hand the chunks to another process (the downstream search) through a shared-memory ring
        const std::string ring = ob.per_trial_share(o.dm.ring);
        if (int rc = open_or_refuse(ob.dm_rsink, new dm_ring_sink(ob.shard, n_freq, ob.my_trials, ob.my_dmax, ob.rows_per_block(), ring.c_str(), 4, o.run.gpu, ob.my_first), ring,
                                    "could not create ring %s"))
            return rc;
        oopt.dm_sink = ob.dm_rsink.get();
    }
    return 0;
}

// -S [-C]: the single-pulse search; --events / --stamps / --voltages behind it
int wire_search(observation& ob)
{
    const options& o = ob.o;
    observation_options& oopt = ob.oopt;
    if (!o.sps.on || !ob.dm_here) return 0;
    oopt.sps_widths = o.sps.widths;
    oopt.sps_threshold = o.sps.snr;
    ob.cand_path = ob.per_trial_share(o.sps.cand_path);
    ob.events_path = ob.per_trial_share(o.evt.path);
    ob.stamps_path = ob.per_trial_share(o.evt.stamps_path);
    if (!ob.cand_path.empty()) {
        if (int rc = open_or_refuse(ob.cand_sink, new sps_file_sink(ob.cand_path.c_str()), ob.cand_path)) return rc;
        oopt.sps_sink = ob.cand_sink.get();
    }
    if (ob.events_path.empty()) return 0;
    if (int rc = open_or_refuse(ob.event_sink, new event_file_sink(ob.events_path.c_str()), ob.events_path)) return rc;
    oopt.evt = &o.evt.opt;
    oopt.event_sink = ob.event_sink.get();
    oopt.stamp_bins = o.evt.stamp_bins;
    oopt.stamp_tbin = o.evt.stamp_tbin;
    oopt.stamp_fbin = o.evt.stamp_fbin;
    oopt.stamp_flagged = o.evt.stamp_flagged;
    if (!ob.stamps_path.empty()) {
        stamp_file_sink* s = new stamp_file_sink(ob.stamps_path.c_str(), ob.band.n_freq / o.evt.stamp_fbin, o.evt.stamp_bins, o.evt.stamp_fbin);
        if (int rc = open_or_refuse(ob.stamp_sink, s, ob.stamps_path)) return rc;
        oopt.stamp_sink = ob.stamp_sink.get();
    }
    if (!o.vcut.path.empty()) {
        if (int rc = open_or_refuse(ob.vcut_sink, new voltage_file_sink(o.vcut.path.c_str(), ob.shard, o.vcut.units, 0), o.vcut.path)) return rc;
        oopt.vcut_sink = ob.vcut_sink.get();
        oopt.vcut_units = o.vcut.units;
        oopt.vcut_history_units = o.vcut.history;
        oopt.vcut_flagged = o.vcut.flagged;
    }
    return 0;
}

// -n [-z] [-U] [-F]: the conditioner
int wire_conditioner(observation& ob)
{
    const options& o = ob.o;
    if (!o.cond.given || !ob.dm_here) return 0;
    ob.oopt.cond_baseline = o.cond.pushes;
    ob.oopt.cond_zero_dm = o.cond.zero_dm;
    ob.oopt.cond_auto_threshold = o.cond.auto_threshold;
    const std::vector<uint8_t>& mask = ob.in.cond_mask;
    if (!mask.empty() && (int)mask.size() != ob.band.n_freq)   // (-F was checked against the production band)
        return refuse("-F: the mask has %zu channels, the band of this run %d", mask.size(), ob.band.n_freq);
    ob.oopt.cond_mask = mask.empty() ? nullptr : mask.data();
    return 0;
}

// --fold: the pulsar folder, the k-th --fold-dm dedispersing the k-th pulsar
int wire_folder(observation& ob)
{
    const options& o = ob.o;
    observation_options& oopt = ob.oopt;
    if (o.fold.pulsars.empty() || !ob.dm_here) return 0;
    const int n_psr = (int)o.fold.pulsars.size(), n_freq = ob.band.n_freq;
    std::vector<double> dms((size_t)n_psr, 0.0);
    for (size_t k = 0; k < o.fold.dms.size(); k++) dms[k] = o.fold.dms[k];
    ob.fold_delays.resize((size_t)n_psr * n_freq);
    dm_delays(dms.data(), n_psr, ob.freq.data(), n_freq, ob.freq[0], o.dm.tsamp_ms, ob.fold_delays.data());
    ob.fold_models.resize((size_t)n_psr);
    for (int k = 0; k < n_psr; k++) {
        const fold_spec& p = o.fold.pulsars[(size_t)k];
        if (bf_psr_model_from_spin(p.f0, p.f1, p.phase0, o.dm.tsamp_ms * 1e-3, 0, &ob.fold_models[(size_t)k]) != BF_OK) return refuse("--fold %d: %s", k, bf_last_error());
    }
    oopt.psr_models = ob.fold_models.data();
    oopt.psr_delays = ob.fold_delays.data();
    oopt.n_psr = n_psr;
    oopt.psr_bins = o.fold.bins;
    oopt.psr_dump_rows = o.fold.rows > 0 ? o.fold.rows : ob.rows_per_block();
    if (!o.fold.path.empty()) {
        const std::string path = ob.per_trial_share(o.fold.path);
        if (int rc = open_or_refuse(ob.fold_sink, new psr_file_sink(path.c_str(), n_psr, n_freq, o.fold.bins, ob.shard.n_beams), path)) return rc;
        oopt.psr_sink = ob.fold_sink.get();
    }
    std::cout << "Pulsar folder: " << n_psr << " pulsars, " << o.fold.bins << " bins, a dump every " << oopt.psr_dump_rows << " rows of " << o.dm.tsamp_ms << " ms" << std::endl;
    return 0;
}

// --inject / --inject-train: the plan of the pulses, each at the delays of its own DM (as --fold-dm takes them) and with its nearest trial
// of the whole ladder; --inject-out: one line of truth per pulse
int wire_injector(observation& ob)
{
    const options& o = ob.o;
    if (!o.inj.on() || !ob.dm_here) return 0;
    const int n_f = ob.band.n_freq, n_b = ob.shard.n_beams;
    FILE* truth = nullptr;
    if (!o.inj.path.empty()) {
        const std::string path = ob.per_trial_share(o.inj.path);
        truth = fopen(path.c_str(), "w");
        if (!truth) return refuse("could not open %s", path.c_str());
        fprintf(truth, "# id kind t0|f0 dm trial beam fluence|amp sigma|duty w|bins [t_lo t_hi]\n");
    }
    auto delays_of = [&](double dm, std::vector<int32_t>* d, int* trial) {
        d->resize((size_t)n_f);
        dm_delays(&dm, 1, ob.freq.data(), n_f, ob.freq[0], o.dm.tsamp_ms, d->data());
        return bf_inj_nearest_trial(ob.delays.data(), ob.n_dm, n_f, d->data(), trial);
    };
    bool ok = true;
    uint64_t id = 0;
    for (const inject_spec& sp : o.inj.bursts) {
        inj_plan::burst b;
        int trial = -1;
        b.t0 = (int64_t)sp.v[0];
        b.W = (int)sp.v[5];
        ok = ok && sp.v[2] < n_b && delays_of(sp.v[1], &b.delay, &trial) == BF_OK;
        b.profile.resize((size_t)n_f * (size_t)b.W);
        const std::vector<double> fluence((size_t)n_f, sp.v[3]);
        ok = ok && bf_inj_burst_profile(n_f, b.W, (b.W - 1) / 2.0, sp.v[4], nullptr, fluence.data(), b.profile.data()) == BF_OK;
        b.response.assign((size_t)n_b, 0.0f);
        if (ok) b.response[(size_t)sp.v[2]] = 1.0f;
        if (ok && truth)
            fprintf(truth, "%llu burst %lld %.17g %d %d %.17g %.17g %d %lld %lld\n", (unsigned long long)id, (long long)b.t0, sp.v[1], trial, (int)sp.v[2],
                    sp.v[3], sp.v[4], b.W, (long long)b.t0, (long long)b.t0 + b.W - 1);
        id++;
        ob.inj.bursts.push_back(std::move(b));
    }
    for (const inject_spec& sp : o.inj.trains) {
        inj_plan::train t;
        int trial = -1;
        t.n_bins = (int)sp.v[5];
        ok = ok && sp.v[2] < n_b && delays_of(sp.v[1], &t.delay, &trial) == BF_OK;
        ok = ok && bf_psr_model_from_spin(sp.v[0], 0.0, 0.0, o.dm.tsamp_ms * 1e-3, 0, &t.model) == BF_OK;
        const int on = std::max(1, (int)std::lround(sp.v[4] * t.n_bins));
        t.profile.assign((size_t)n_f * (size_t)t.n_bins, 0.0f);
        for (int f = 0; f < n_f; f++)
            for (int j = 0; j < on; j++) t.profile[(size_t)f * (size_t)t.n_bins + (size_t)j] = (float)sp.v[3];
        t.response.assign((size_t)n_b, 0.0f);
        if (ok) t.response[(size_t)sp.v[2]] = 1.0f;
        if (ok && truth)
            fprintf(truth, "%llu train %.17g %.17g %d %d %.17g %.17g %d\n", (unsigned long long)id, sp.v[0], sp.v[1], trial, (int)sp.v[2], sp.v[3], sp.v[4], t.n_bins);
        id++;
        ob.inj.trains.push_back(std::move(t));
    }
    if (truth) fclose(truth);
    if (!ok)
        return refuse("--inject / --inject-train: BEAM must be below the %d beams of this run, and the pulse must fit its window (%s)", n_b, bf_last_error());
    ob.oopt.inj = &ob.inj;
    std::cout << "Injector: " << ob.inj.bursts.size() << " bursts and " << ob.inj.trains.size() << " trains in front of the DM stage" << std::endl;
    return 0;
}

// --ffa: the periodicity search
int wire_ffa(observation& ob)
{
    const options& o = ob.o;
    observation_options& oopt = ob.oopt;
    if (!o.ffa.on || !ob.dm_here) return 0;
    oopt.ffa_p_lo = o.ffa.p_lo;
    oopt.ffa_p_hi = o.ffa.p_hi;
    oopt.ffa_seg = o.ffa.seg;
    oopt.ffa_dec = o.ffa.dec;
    oopt.ffa_oct = o.ffa.oct;
    oopt.ffa_widths = o.ffa.widths;
    oopt.ffa_threshold = o.ffa.snr;
    oopt.ffa_detrend_blk = o.ffa.detrend_blk;
    oopt.ffa_detrend_win = o.ffa.detrend_win;
    ob.ffa_path = ob.per_trial_share(o.ffa.path);
    if (ob.ffa_path.empty()) return 0;
    ffa_file_sink* s = new ffa_file_sink(ob.ffa_path.c_str(), o.ffa.dec, o.ffa.seg, o.ffa.oct, o.ffa.p_lo, o.ffa.p_hi, o.ffa.widths, o.ffa.snr, o.ffa.detrend_blk, o.ffa.detrend_win);
    if (int rc = open_or_refuse(ob.ffa_sink, s, ob.ffa_path)) return rc;
    oopt.ffa_sink = ob.ffa_sink.get();
    return 0;
}

// -V, -Y, -x: the correlator, the voltage moments and the Stokes beams -- every shard works on its own channels
int wire_voltage_products(observation& ob)
{
    const options& o = ob.o;
    observation_options& oopt = ob.oopt;
    if (!o.corr.path.empty()) {
        ob.vis_path = ob.per_shard(o.corr.path);
        if (int rc = open_or_refuse(ob.vis_sink, new vis_file_sink(ob.shard, ob.vis_path.c_str(), ob.first_channel(), o.run.gpu), ob.vis_path)) return rc;
        oopt.corr_blocks = o.corr.blocks;
        oopt.vis_sink = ob.vis_sink.get();
    }
    if (!o.sk.path.empty()) {
        ob.sk_path = ob.per_shard(o.sk.path);
        if (int rc = open_or_refuse(ob.sk_sink, new sk_file_sink(ob.shard, ob.sk_path.c_str(), ob.first_channel(), o.run.gpu), ob.sk_path)) return rc;
        oopt.sk_blocks = o.sk.blocks;
        oopt.sk_sink = ob.sk_sink.get();
    }
    if (!o.stokes.path.empty()) {
        ob.stokes_path = ob.per_shard(o.stokes.path);
        const int n_int = o.stokes.int_given ? o.stokes.n_int : ob.shard.n_avg;
        stokes_file_sink* s = new stokes_file_sink(ob.shard, ob.stokes_path.c_str(), ob.first_channel(), o.run.gpu, o.stokes.beams, n_int);
        if (int rc = open_or_refuse(ob.stokes_sink, s, ob.stokes_path)) return rc;
        oopt.stokes_beams = o.stokes.beams;
        oopt.stokes_int = n_int;
        oopt.stokes_sink = ob.stokes_sink.get();
    }
    return 0;
}

int run_observe(const options& o, const inputs& in)
{
    observation ob(o, in);
    if (int rc = join_shards(ob)) return rc;
    std::vector<antenna> pos;
    std::vector<beam_direction> dir;
    read_layout(o, ob.shard.n_ant, ob.shard.n_beams, &pos, &dir);
    for (int (*step)(observation&) : {open_source, open_detected_sink, plan_dm_stage, wire_search, wire_conditioner, wire_folder, wire_injector, wire_ffa, wire_voltage_products})
        if (int rc = step(ob)) return rc;
    observation_result result;
    const int rc = run_observation(ob.shard, ob.oopt, *ob.src, pos.data(), dir.data(), &result, std::cout);
    if (ob.sink) std::cout << "Wrote " << ob.sink->get_delivered() << " gemm-units of detected powers to " << ob.sink_name << std::endl;
    if (ob.dm_sink) std::cout << "Wrote " << ob.dm_sink->get_times_written() << " dedispersed samples x " << ob.my_trials << " trials to " << ob.dm_path << std::endl;
    if (ob.cand_sink) std::cout << "Wrote " << ob.cand_sink->get_candidates_written() << " candidates to " << ob.cand_path << std::endl;
    if (ob.ffa_sink) std::cout << "Wrote " << ob.ffa_sink->get_candidates_written() << " periodicity candidates to " << ob.ffa_path << std::endl;
    if (ob.event_sink) std::cout << "Wrote " << ob.event_sink->get_events_written() << " events to " << ob.events_path << std::endl;
    if (ob.stamp_sink) std::cout << "Wrote " << ob.stamp_sink->get_stamps_written() << " stamps to " << ob.stamps_path << std::endl;
    if (ob.vcut_sink) std::cout << "Wrote " << ob.vcut_sink->get_cuts_written() << " voltage cuts to " << o.vcut.path << std::endl;
    if (ob.vis_sink) std::cout << "Wrote " << ob.vis_sink->get_dumps_written() << " visibility dumps of " << o.corr.blocks << " blocks to " << ob.vis_path << std::endl;
    if (ob.stokes_sink) std::cout << "Wrote " << ob.stokes_sink->get_sets_written() << " sets of Stokes beams to " << ob.stokes_path << std::endl;
    if (ob.sk_sink) std::cout << "Wrote " << ob.sk_sink->get_dumps_written() << " moment dumps of " << o.sk.blocks << " blocks to " << ob.sk_path << std::endl;
    bf_comm_destroy(ob.comm);
    return rc == BF_OK ? 0 : gpu_assert(rc);
}

}  // namespace

int main(int argc, char* argv[])
{
    options o;
    inputs in;
    if (int rc = parse(argc, argv, o); rc >= 0) return rc;
    if (int rc = check(o, &in)) return rc;
    if (!o.select.path.empty()) return run_select(o);   // host only
    if (int rc = load(o, &in)) return rc;

    int n_dev = 0;
    if (bf_device_count(&n_dev) != BF_OK || n_dev == 0) {
        fprintf(stderr, "GPUassert: %s\n", bf_last_error());  // src/beamformer.cuh:26
        return EXIT_FAILURE;
    }
    char name[256];
    if (bf_device_name(o.run.device, name, sizeof name) == BF_OK) std::cout << "Selected: " << name << std::endl;

    if (!o.solve.vis.empty()) return run_solve(o, in);
    if (!o.coherent.path.empty()) return run_coherent(o, in);
    if (!o.faraday.path.empty()) return run_faraday(o, in);
    if (o.observe()) return run_observe(o, in);
    return run_debug(o, in);
}
