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
#include <cstdio>
#include <fstream>
#include <thread>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dsabf_host.hpp"

int main(int argc, char* argv[])
{
    using namespace dsabf;
    bf_config cfg;
    bf_config_default(&cfg, /*debug=*/1);
    debug_run_options opt;
    bool per_unit = false;
    std::string positions, directions, sources, output = "bin/data.py", detected_path, out_ring;
    std::string ring_key;
    int core = -1;
    long junk_blocks = -1;
    int world = 1, rank = 0;
    std::string id_file;
    double dm_max = 0.0, tsamp_ms = 0.131;   // (the notebook's sample time, cell 5)
    int n_dm_cap = 0;
    bool dm_split = false;
    std::string dm_path, dm_ring;   // -W file / -Q shared-memory ring for the DM chunks
    double sps_snr = 0.0;           // -S: threshold of the single-pulse search (0: off)
    int sps_widths = 6;             // -B
    bool sps_on = false, sps_widths_given = false;
    std::string cand_path;          // -C
    int cond_n = 0;                 // -n: the conditioner's window in pushes (0: no conditioner)
    bool cond_given = false, cond_zdm = false, cond_auto_given = false;   // -z: zero-DM (off in the driver unless given)
    double cond_auto = 0.0;         // -U
    std::string cond_mask_path;     // -F
    int ib_beam = -1;               // -i: the beam column that carries the incoherent beam (-1: none)
    bool ib_given = false;
    std::string vis_path;           // -V: where the correlator's dumps go
    int corr_blocks = 1;            // -L: analysed blocks integrated per dump
    bool corr_blocks_given = false;
    std::string solve_vis, solve_gains_path, apply_gains;   // -E / -G: the gain solver on a -V file; -A: gains applied to the weights
    bool solve_joint = false;                               // -P
    std::string sk_path;            // -Y: where the voltage moments go
    int sk_blocks = 1;              // -J: analysed blocks integrated per dump
    bool sk_blocks_given = false;
    std::string select_path, select_ant_path, select_chan_path;   // -e / -O / -q: flags from a -Y file
    bf_sk_options sk_opt;           // -t n_sigma, -m centre
    bf_sk_default_options(&sk_opt);
    bool sk_sigma_given = false, sk_centre_given = false;
    std::string ant_flags_path;     // -f: antenna flags for -E, -A or -Z
    std::string null_path, null_spec;   // -Z: the null file (written with -E, applied otherwise); -y n_null[:min_ratio]
    bf_null_options null_opt;
    bf_null_default_options(&null_opt);
    std::string stokes_path, stokes_list;   // -x: where the Stokes beams go; -b: the beams to follow
    int stokes_int = 0;                     // -l: samples per integration window (0: N_AVERAGING)
    bool stokes_int_given = false;

    // events and stamps (docs/EVENTS.md): long options only -- every letter is taken
    std::string events_path, stamps_path;   // --events FILE, --stamps FILE
    bf_evt_options evt_opt;
    bf_evt_default_options(&evt_opt);
    int stamp_bins = 64, stamp_tbin = 0, stamp_fbin = 1;
    bool event_tol_given = false, event_veto_given = false, stamp_shape_given = false, stamp_flagged = false, long_bad = false;
    // voltage cuts (docs/VOLTAGE_CUTS.md): --voltages FILE [--voltage-units N] [--voltage-history UNITS] [--voltage-flagged]
    std::string voltages_path;
    int voltage_units = 2, voltage_history = 0;
    bool voltage_units_given = false, voltage_history_given = false, voltage_flagged = false, voltage_bad = false;
    // coherent dedispersion of a --voltages file (docs/COHERENT_DEDISPERSION.md): --coherent V_FILE --coherent-out FILE [--coherent-fft N]
    // [--coherent-int n] [--coherent-sideband +1|-1]; no observation is run
    std::string coherent_path, coherent_out;
    int coherent_fft = 0, coherent_int = 1, coherent_sideband = 1;
    bool coherent_extra_given = false, coherent_bad = false;
    // pulsar folding (docs/PULSAR_FOLDING.md): --fold f0[:f1[:phase0]] up to 4 times, --fold-dm dm (the k-th belongs to the k-th --fold),
    // --fold-bins n, --fold-rows rows_per_dump, --fold-out FILE
    struct fold_spec {
        double f0 = 0.0, f1 = 0.0, phase0 = 0.0, dm = 0.0;
    };
    std::vector<fold_spec> folds;
    std::vector<double> fold_dms;
    int fold_bins = 64, fold_rows = 0;
    std::string fold_path;
    bool fold_extra_given = false, fold_bad = false;
    // periodicity search (docs/PERIODICITY.md): --ffa p_lo:p_hi, --ffa-seg n_seg, --ffa-dec tdec, --ffa-oct n, --ffa-widths K, --ffa-snr threshold,
    // --ffa-out FILE, --ffa-detrend blk:win
    int ffa_p_lo = 0, ffa_p_hi = 0, ffa_seg = 1024, ffa_dec = 1, ffa_oct = 1, ffa_widths = 3, ffa_det_blk = 0, ffa_det_win = 0;
    double ffa_snr = 8.0;
    std::string ffa_path;
    bool ffa_given = false, ffa_extra_given = false, ffa_bad = false;
    // pulse injection (docs/INJECTION.md): --inject t0:dm:beam:fluence[:sigma[:w]] any number of times, --inject-train f0:dm:beam:amp[:duty[:bins]]
    // up to 4 times, --inject-out FILE (one line of truth per pulse)
    struct inject_spec {
        double v[6] = {0, 0, 0, 0, 0, 0};
        int n = 0;   // fields given
    };
    std::vector<inject_spec> inj_bursts, inj_trains;
    std::string inj_path;
    bool inj_bad = false;
    enum { kEvents = 1000, kEventTol, kEventVeto, kStamps, kStampShape, kStampFlagged, kFold, kFoldDm, kFoldBins, kFoldRows, kFoldOut, kFfa, kFfaSeg, kFfaDec, kFfaOct, kFfaWidths, kFfaSnr, kFfaOut, kFfaDetrend, kInject, kInjectTrain, kInjectOut, kVoltages, kVoltageUnits, kVoltageHistory, kVoltageFlagged, kCoherent, kCoherentOut, kCoherentFft, kCoherentInt, kCoherentSideband };
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
                                          {nullptr, 0, nullptr, 0}};
    // a non-negative integer that fills its whole field; anything else marks the command line as malformed
    auto number = [&long_bad](const char* text, const char** end, int* out) {
        char* e = nullptr;
        const long v = strtol(text, &e, 10);
        if (e == text || v < 0 || v > 1000000000L || *text == '-' || *text == '+' || *text == ' ') long_bad = true;
        *out = (int)v;
        *end = e;
    };

    int arg = 0;
    while ((arg = getopt_long(argc, argv, "s:g:p:d:o:D:a:c:k:K:j:w:R:r:I:M:N:T:W:Q:S:B:C:i:V:L:E:G:A:n:U:F:Y:J:e:O:q:t:m:f:x:b:l:Z:y:zPXuvhH", long_options, nullptr)) != -1) {  // src/beamformer.cu:41-43 (+ -o -D -a -v)
        switch (arg) {
            case kFold: {   // f0[:f1[:phase0]]
                fold_spec fs;
                double* field[3] = {&fs.f0, &fs.f1, &fs.phase0};
                const char* at = optarg;
                for (int i = 0; i < 3; i++) {
                    char* e = nullptr;
                    *field[i] = strtod(at, &e);
                    if (e == at) fold_bad = true;
                    at = e;
                    if (*at != ':') break;
                    at++;
                    if (i == 2) fold_bad = true;
                }
                if (*at) fold_bad = true;
                folds.push_back(fs);
                break;
            }
            case kInject:
            case kInjectTrain: {   // four to six numbers between colons
                inject_spec sp;
                const char* at = optarg;
                for (;;) {
                    char* e = nullptr;
                    const double v = strtod(at, &e);
                    if (e == at || sp.n == 6 || !std::isfinite(v)) {
                        inj_bad = true;
                        break;
                    }
                    sp.v[sp.n++] = v;
                    at = e;
                    if (*at != ':') break;
                    at++;
                }
                if (*at || sp.n < 4) inj_bad = true;
                (arg == kInject ? inj_bursts : inj_trains).push_back(sp);
                break;
            }
            case kInjectOut: inj_path = optarg; break;
            case kFoldDm: {
                char* e = nullptr;
                fold_dms.push_back(strtod(optarg, &e));
                if (e == optarg || *e || !(fold_dms.back() >= 0.0)) fold_bad = true;
                fold_extra_given = true;
                break;
            }
            case kFoldBins:
            case kFoldRows: {
                const char* e = nullptr;
                bool bad = long_bad;
                long_bad = false;
                number(optarg, &e, arg == kFoldBins ? &fold_bins : &fold_rows);
                if (*e || long_bad) fold_bad = true;
                long_bad = bad;
                fold_extra_given = true;
                break;
            }
            case kFoldOut:
                fold_path = optarg;
                fold_extra_given = true;
                break;
            case kFfa: {   // p_lo:p_hi
                const char* e = nullptr;
                bool bad = long_bad;
                long_bad = false;
                number(optarg, &e, &ffa_p_lo);
                if (*e == ':')
                    number(e + 1, &e, &ffa_p_hi);
                else
                    ffa_bad = true;
                if (*e || long_bad) ffa_bad = true;
                long_bad = bad;
                ffa_given = true;
                break;
            }
            case kFfaDetrend: {   // blk:win
                const char* e = nullptr;
                bool bad = long_bad;
                long_bad = false;
                number(optarg, &e, &ffa_det_blk);
                if (*e == ':')
                    number(e + 1, &e, &ffa_det_win);
                else
                    ffa_bad = true;
                if (*e || long_bad) ffa_bad = true;
                long_bad = bad;
                ffa_extra_given = true;
                break;
            }
            case kFfaSeg:
            case kFfaDec:
            case kFfaOct:
            case kFfaWidths: {
                const char* e = nullptr;
                bool bad = long_bad;
                long_bad = false;
                number(optarg, &e, arg == kFfaSeg ? &ffa_seg : arg == kFfaDec ? &ffa_dec : arg == kFfaOct ? &ffa_oct : &ffa_widths);
                if (*e || long_bad) ffa_bad = true;
                long_bad = bad;
                ffa_extra_given = true;
                break;
            }
            case kFfaSnr: {
                char* e = nullptr;
                ffa_snr = strtod(optarg, &e);
                if (e == optarg || *e || !(ffa_snr == ffa_snr)) ffa_bad = true;
                ffa_extra_given = true;
                break;
            }
            case kFfaOut:
                ffa_path = optarg;
                ffa_extra_given = true;
                break;
            case kEvents: events_path = optarg; break;
            case kStamps: stamps_path = optarg; break;
            case kStampFlagged: stamp_flagged = true; break;
            case kVoltages: voltages_path = optarg; break;
            case kVoltageFlagged: voltage_flagged = true; break;
            case kCoherent: coherent_path = optarg; break;
            case kCoherentOut: coherent_out = optarg; break;
            case kCoherentFft:
            case kCoherentInt:
            case kCoherentSideband: {   // a whole number that fills its field
                char* e = nullptr;
                const long v = strtol(optarg, &e, 10);
                if (e == optarg || *e || v < -1000000000L || v > 1000000000L || *optarg == ' ') coherent_bad = true;
                (arg == kCoherentFft ? coherent_fft : arg == kCoherentInt ? coherent_int : coherent_sideband) = (int)v;
                coherent_extra_given = true;
                break;
            }
            case kVoltageUnits:
            case kVoltageHistory: {   // a whole number >= 1
                char* e = nullptr;
                const long v = strtol(optarg, &e, 10);
                if (e == optarg || *e || v < 1 || v > 1000000000L || *optarg == '+' || *optarg == ' ') voltage_bad = true;
                (arg == kVoltageUnits ? voltage_units : voltage_history) = (int)v;
                (arg == kVoltageUnits ? voltage_units_given : voltage_history_given) = true;
                break;
            }
            case kEventTol: {   // T[,D]
                const char* e = nullptr;
                event_tol_given = true;
                number(optarg, &e, &evt_opt.t_tol);
                if (*e == ',') number(e + 1, &e, &evt_opt.dm_tol);
                if (*e) long_bad = true;
                break;
            }
            case kEventVeto: {   // MAXBEAMS[:IB_RATIO]
                const char* e = nullptr;
                event_veto_given = true;
                number(optarg, &e, &evt_opt.max_beams);
                if (*e == ':') {
                    char* e2 = nullptr;
                    evt_opt.ib_ratio = strtod(e + 1, &e2);
                    if (e2 == e + 1 || *e2 || !(evt_opt.ib_ratio >= 0.0)) long_bad = true;
                    e = e2;
                }
                if (*e) long_bad = true;
                break;
            }
            case kStampShape: {   // BINS[:TBIN[:FBIN]]
                const char* e = nullptr;
                stamp_shape_given = true;
                number(optarg, &e, &stamp_bins);
                if (*e == ':') number(e + 1, &e, &stamp_tbin);
                if (*e == ':') number(e + 1, &e, &stamp_fbin);
                if (*e || stamp_bins < 1 || stamp_fbin < 1) long_bad = true;
                break;
            }
            case 's': sources = optarg; break;                 // :77-89
            case 'g': opt.gpu = atoi(optarg); break;           // :92-100
            case 'p': positions = optarg; break;               // :102-111
            case 'd': directions = optarg; break;              // :113-121
            case 'o': output = optarg; break;
            case 'D': opt.device = atoi(optarg); break;
            case 'a': cfg.n_avg = atoi(optarg); break;
            case 'j': junk_blocks = atol(optarg); break;
            case 'w': detected_path = optarg; break;
            case 'K': out_ring = optarg; break;
            case 'R': world = atoi(optarg); break;
            case 'r': rank = atoi(optarg); break;
            case 'I': id_file = optarg; break;
            case 'M': dm_max = atof(optarg); break;
            case 'N': n_dm_cap = atoi(optarg); break;
            case 'T': tsamp_ms = atof(optarg); break;
            case 'W': dm_path = optarg; break;
            case 'X': dm_split = true; break;
            case 'Q': dm_ring = optarg; break;
            case 'S': sps_snr = atof(optarg); sps_on = true; break;
            case 'B': sps_widths = atoi(optarg); sps_widths_given = true; break;
            case 'C': cand_path = optarg; break;
            case 'n': cond_n = atoi(optarg); cond_given = true; break;
            case 'z': cond_zdm = true; break;
            case 'U': cond_auto = atof(optarg); cond_auto_given = true; break;
            case 'F': cond_mask_path = optarg; break;
            case 'i': ib_beam = atoi(optarg); ib_given = true; break;
            case 'V': vis_path = optarg; break;
            case 'L': corr_blocks = atoi(optarg); corr_blocks_given = true; break;
            case 'E': solve_vis = optarg; break;
            case 'G': solve_gains_path = optarg; break;
            case 'A': apply_gains = optarg; break;
            case 'P': solve_joint = true; break;
            case 'Y': sk_path = optarg; break;
            case 'J': sk_blocks = atoi(optarg); sk_blocks_given = true; break;
            case 'e': select_path = optarg; break;
            case 'O': select_ant_path = optarg; break;
            case 'q': select_chan_path = optarg; break;
            case 't': sk_opt.n_sigma = atof(optarg); sk_sigma_given = true; break;
            case 'm': sk_opt.centre = atof(optarg); sk_centre_given = true; break;
            case 'f': ant_flags_path = optarg; break;
            case 'Z': null_path = optarg; break;
            case 'y': null_spec = optarg; break;
            case 'x': stokes_path = optarg; break;
            case 'b': stokes_list = optarg; break;
            case 'l': stokes_int = atoi(optarg); stokes_int_given = true; break;
            case 'u': per_unit = true; break;                   // the reference's launch pattern: one launch per gemm-unit
            case 'v': opt.verbose = true; cfg.verbose = 1; break;
            case 'c': core = atoi(optarg); break;              // :59-65
            case 'k': ring_key = optarg; break;                // :66-75 (a shared-memory ring name instead of a hex key)
            case 'h': usage(true, std::cout); return EXIT_SUCCESS;  // :123-125
            case 'H':   // the reference's text, then what this build adds to its command line
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
                return EXIT_SUCCESS;
            default: usage(true, std::cerr); return EXIT_FAILURE;
        }
    }
    if (sps_on && !(dm_max > 0.0)) {
        fprintf(stderr, "beam: -S (single-pulse search) requires the DM stage: give -M dm_max\n");
        return EXIT_FAILURE;
    }
    if (!sps_on && (sps_widths_given || !cand_path.empty())) {
        fprintf(stderr, "beam: -B / -C belong to the single-pulse search: give -S snr (and -M dm_max)\n");
        return EXIT_FAILURE;
    }
    if (!folds.empty() && !(dm_max > 0.0)) {
        fprintf(stderr, "beam: --fold (pulsar folding) requires the DM stage: give -M dm_max\n");
        return EXIT_FAILURE;
    }
    if (folds.empty() && fold_extra_given) {
        fprintf(stderr, "beam: --fold-dm / --fold-bins / --fold-rows / --fold-out belong to the pulsar folder: give --fold F0[:F1[:PHASE0]]\n");
        return EXIT_FAILURE;
    }
    if (fold_bad || folds.size() > (size_t)BF_PSR_MAX_PULSARS || fold_dms.size() > folds.size() ||
        (!folds.empty() && (fold_bins < 2 || fold_bins > BF_PSR_MAX_BINS || fold_rows < 0))) {
        fprintf(stderr, "beam: --fold F0[:F1[:PHASE0]] (at most %d), --fold-dm DM >= 0 (one per --fold at most), --fold-bins 2 .. %d, --fold-rows ROWS: "
                        "malformed, too many or out of range\n", BF_PSR_MAX_PULSARS, BF_PSR_MAX_BINS);
        return EXIT_FAILURE;
    }
    const bool inj_given = !inj_bursts.empty() || !inj_trains.empty();
    if ((inj_given || !inj_path.empty()) && !(dm_max > 0.0)) {
        fprintf(stderr, "beam: --inject / --inject-train / --inject-out (pulse injection) require the DM stage: give -M dm_max\n");
        return EXIT_FAILURE;
    }
    if (!inj_given && !inj_path.empty()) {
        fprintf(stderr, "beam: --inject-out belongs to the pulse injection: give --inject T0:DM:BEAM:FLUENCE or --inject-train F0:DM:BEAM:AMP\n");
        return EXIT_FAILURE;
    }
    {   // the ranges that need no geometry: whole numbers where whole numbers go, DM >= 0, SIGMA > 0, W and BINS within the stage's bounds
        auto whole = [](double v, double lo, double hi) { return v >= lo && v <= hi && v == std::floor(v); };
        for (inject_spec& sp : inj_bursts) {
            if (sp.n < 5) sp.v[4] = 1.0;
            if (sp.n < 6) {
                double w = 1.0;
                while (w < 8.0 * sp.v[4] && w <= (double)BF_INJ_MAX_WIDTH) w *= 2.0;
                sp.v[5] = w;
            }
            if (!whole(sp.v[0], 0, 9e15) || !(sp.v[1] >= 0.0) || !whole(sp.v[2], 0, 1e9) || !(sp.v[4] > 0.0) || !whole(sp.v[5], 1, BF_INJ_MAX_WIDTH)) inj_bad = true;
        }
        for (inject_spec& sp : inj_trains) {
            if (sp.n < 5) sp.v[4] = 0.05;
            if (sp.n < 6) sp.v[5] = 64.0;
            if (!(sp.v[1] >= 0.0) || !whole(sp.v[2], 0, 1e9) || !(sp.v[4] > 0.0 && sp.v[4] <= 1.0) || !whole(sp.v[5], 2, BF_PSR_MAX_BINS)) inj_bad = true;
        }
    }
    if (inj_bad || inj_trains.size() > (size_t)BF_INJ_MAX_TRAINS || inj_bursts.size() + inj_trains.size() > (size_t)BF_INJ_MAX_PULSES) {
        fprintf(stderr, "beam: --inject T0:DM:BEAM:FLUENCE[:SIGMA[:W]], --inject-train F0:DM:BEAM:AMP[:DUTY[:BINS]] (at most %d): malformed, too many or out of range\n",
                BF_INJ_MAX_TRAINS);
        return EXIT_FAILURE;
    }
    if (ffa_given && !(dm_max > 0.0)) {
        fprintf(stderr, "beam: --ffa (periodicity search) requires the DM stage: give -M dm_max\n");
        return EXIT_FAILURE;
    }
    if (!ffa_given && ffa_extra_given) {
        fprintf(stderr, "beam: --ffa-seg / --ffa-dec / --ffa-oct / --ffa-widths / --ffa-snr / --ffa-out / --ffa-detrend belong to the periodicity search: give --ffa P_LO:P_HI\n");
        return EXIT_FAILURE;
    }
    if (ffa_bad) {
        fprintf(stderr, "beam: --ffa P_LO:P_HI, --ffa-seg N, --ffa-dec N, --ffa-oct N, --ffa-widths N, --ffa-snr SNR, --ffa-detrend BLK:WIN: malformed number\n");
        return EXIT_FAILURE;
    }
    if (long_bad) {
        fprintf(stderr, "beam: --event-tol T[,D], --event-veto MAXBEAMS[:IB_RATIO], --stamp-shape BINS[:TBIN[:FBIN]]: malformed or negative number\n");
        return EXIT_FAILURE;
    }
    if (!events_path.empty() && !sps_on) {
        fprintf(stderr, "beam: --events groups the candidates of the single-pulse search: give -S snr (and -M dm_max)\n");
        return EXIT_FAILURE;
    }
    if (events_path.empty() && (event_tol_given || event_veto_given || !stamps_path.empty())) {
        fprintf(stderr, "beam: --event-tol / --event-veto / --stamps belong to the event builder: give --events FILE\n");
        return EXIT_FAILURE;
    }
    if (stamps_path.empty() && (stamp_shape_given || stamp_flagged)) {
        fprintf(stderr, "beam: --stamp-shape / --stamp-flagged belong to the stamps: give --stamps FILE\n");
        return EXIT_FAILURE;
    }
    if (voltage_bad) {
        fprintf(stderr, "beam: --voltage-units N, --voltage-history UNITS: need a whole number >= 1\n");
        return EXIT_FAILURE;
    }
    if (voltages_path.empty() && (voltage_units_given || voltage_history_given || voltage_flagged)) {
        fprintf(stderr, "beam: --voltage-units / --voltage-history / --voltage-flagged belong to the voltage cuts: give --voltages FILE\n");
        return EXIT_FAILURE;
    }
    if (!voltages_path.empty() && events_path.empty()) {
        fprintf(stderr, "beam: --voltages cuts the voltages of the event builder's events: give --events FILE\n");
        return EXIT_FAILURE;
    }
    if (!voltages_path.empty() && world > 1) {
        fprintf(stderr, "beam: --voltages is not available in a sharded run (-R): a trigger is not sent to the ranks that hold the other channels\n");
        return EXIT_FAILURE;
    }
    if (coherent_path.empty() && (!coherent_out.empty() || coherent_extra_given)) {
        fprintf(stderr, "beam: --coherent-out / --coherent-fft / --coherent-int / --coherent-sideband belong to coherent dedispersion: give --coherent V_FILE\n");
        return EXIT_FAILURE;
    }
    if (!coherent_path.empty()) {
        if (junk_blocks >= 0 || !ring_key.empty() || !solve_vis.empty()) {
            fprintf(stderr, "beam: --coherent runs no observation and no solver: leave out -j / -k / -E\n");
            return EXIT_FAILURE;
        }
        if (coherent_out.empty()) {
            fprintf(stderr, "beam: --coherent needs --coherent-out FILE (where the Stokes parameters go)\n");
            return EXIT_FAILURE;
        }
        if (!(dm_max > 0.0)) {
            fprintf(stderr, "beam: --coherent takes the DM of a cut from the ladder of the run that wrote it: give that run's -M dm_max (and -N, -T)\n");
            return EXIT_FAILURE;
        }
        bool pow2 = false;
        for (int n = 64; n <= 4096; n *= 2) pow2 = pow2 || coherent_fft == n;
        if (coherent_bad || (coherent_fft != 0 && !pow2) || coherent_int < 1 || (coherent_sideband != 1 && coherent_sideband != -1)) {
            fprintf(stderr, "beam: --coherent-fft N: a power of two 64 .. 4096; --coherent-int n: a whole number >= 1; --coherent-sideband: +1 or -1\n");
            return EXIT_FAILURE;
        }
        if (!(tsamp_ms > 0.0)) {
            fprintf(stderr, "beam: -T %g: the sample time must be positive\n", tsamp_ms);
            return EXIT_FAILURE;
        }
    }
    if (!stamps_path.empty()) {   // the band is the production geometry's, whatever -R
        bf_config band;
        bf_config_default(&band, /*debug=*/0);
        if (band.n_freq % stamp_fbin != 0) {
            fprintf(stderr, "beam: --stamp-shape: FBIN %d does not divide the band's %d channels\n", stamp_fbin, band.n_freq);
            return EXIT_FAILURE;
        }
    }
    if (sps_on && (sps_widths < 1 || sps_widths > 8)) {
        fprintf(stderr, "beam: -B %d: n_widths must be 1 .. 8\n", sps_widths);
        return EXIT_FAILURE;
    }
    if ((cond_given || cond_zdm || cond_auto_given || !cond_mask_path.empty()) && !(dm_max > 0.0)) {
        fprintf(stderr, "beam: -n / -z / -U / -F (conditioner) require the DM stage: give -M dm_max\n");
        return EXIT_FAILURE;
    }
    if (!cond_given && (cond_zdm || cond_auto_given || !cond_mask_path.empty())) {
        fprintf(stderr, "beam: -z / -U / -F belong to the conditioner: give -n baseline_pushes\n");
        return EXIT_FAILURE;
    }
    if (cond_given && (cond_n < 1 || cond_n > 64)) {
        fprintf(stderr, "beam: -n %d: baseline_pushes must be 1 .. 64\n", cond_n);
        return EXIT_FAILURE;
    }
    if (cond_auto_given && !(cond_auto >= 0.0)) {
        fprintf(stderr, "beam: -U %s: the automatic mask's threshold must be >= 0\n", std::to_string(cond_auto).c_str());
        return EXIT_FAILURE;
    }
    std::vector<uint8_t> cond_mask;   // -F: read before any device is touched; the band is the production geometry's, whatever -R
    if (!cond_mask_path.empty()) {
        bf_config band;
        bf_config_default(&band, /*debug=*/0);
        std::ifstream in(cond_mask_path);
        if (!in) {
            fprintf(stderr, "beam: -F %s: could not be read\n", cond_mask_path.c_str());
            return EXIT_FAILURE;
        }
        cond_mask.assign((size_t)band.n_freq, 0);
        std::string line;
        while (std::getline(in, line)) {
            line = line.substr(0, line.find('#'));
            const size_t a = line.find_first_not_of(" \t\r");
            if (a == std::string::npos) continue;
            char* end = nullptr;
            const long ch = strtol(line.c_str() + a, &end, 10);
            while (*end == ' ' || *end == '\t' || *end == '\r') end++;
            if (end == line.c_str() + a || *end || ch < 0 || ch >= band.n_freq) {
                fprintf(stderr, "beam: -F %s: '%s' is not a channel index 0 .. %d\n", cond_mask_path.c_str(), line.c_str() + a, band.n_freq - 1);
                return EXIT_FAILURE;
            }
            cond_mask[(size_t)ch] = 1;
        }
    }
    if (ib_given && (ib_beam < 0 || ib_beam >= cfg.n_beams)) {
        fprintf(stderr, "beam: -i %d: the incoherent beam takes a beam index 0 .. %d\n", ib_beam, cfg.n_beams - 1);
        return EXIT_FAILURE;
    }
    if (ib_given && junk_blocks < 0 && ring_key.empty()) {
        fprintf(stderr, "beam: -i (incoherent beam) belongs to the observation mode: give -j n_blocks or -k ring\n");
        return EXIT_FAILURE;
    }
    if (corr_blocks_given && vis_path.empty()) {
        fprintf(stderr, "beam: -L (blocks per dump) belongs to the correlator: give -V vis_file\n");
        return EXIT_FAILURE;
    }
    if (corr_blocks_given && corr_blocks < 1) {
        fprintf(stderr, "beam: -L %d: the correlator integrates at least one block per dump\n", corr_blocks);
        return EXIT_FAILURE;
    }
    if (!vis_path.empty() && junk_blocks < 0 && ring_key.empty()) {
        fprintf(stderr, "beam: -V (correlator) belongs to the observation mode: give -j n_blocks or -k ring\n");
        return EXIT_FAILURE;
    }
    const bool observe_mode = junk_blocks >= 0 || !ring_key.empty();
    if (sk_blocks_given && sk_path.empty()) {
        fprintf(stderr, "beam: -J (blocks per dump) belongs to the voltage moments: give -Y moments_file\n");
        return EXIT_FAILURE;
    }
    if (sk_blocks_given && sk_blocks < 1) {
        fprintf(stderr, "beam: -J %d: the moments integrate at least one block per dump\n", sk_blocks);
        return EXIT_FAILURE;
    }
    if (!sk_path.empty() && !observe_mode) {
        fprintf(stderr, "beam: -Y (voltage moments) belongs to the observation mode: give -j n_blocks or -k ring\n");
        return EXIT_FAILURE;
    }
    std::vector<int> stokes_beams;   // -b: parsed before any device is touched
    if (stokes_path.empty() && (!stokes_list.empty() || stokes_int_given)) {
        fprintf(stderr, "beam: -b / -l belong to the Stokes beams: give -x stokes_file\n");
        return EXIT_FAILURE;
    }
    if (!stokes_path.empty()) {
        if (!observe_mode) {
            fprintf(stderr, "beam: -x (Stokes beams) belongs to the observation mode: give -j n_blocks or -k ring\n");
            return EXIT_FAILURE;
        }
        if (stokes_list.empty()) {
            fprintf(stderr, "beam: -x needs -b b0,b1,... (the beams to follow)\n");
            return EXIT_FAILURE;
        }
        bf_config band;   // the observation mode's geometry
        bf_config_default(&band, /*debug=*/0);
        std::string why;
        if (!parse_beam_list(stokes_list.c_str(), band.n_beams, &stokes_beams, &why)) {
            fprintf(stderr, "beam: -b %s\n", why.c_str());
            return EXIT_FAILURE;
        }
        const int samples = band.n_out_per_gemm * band.n_avg;
        if (stokes_int_given && (stokes_int < 1 || samples % stokes_int)) {
            fprintf(stderr, "beam: -l %d: the window must be at least 1 and divide the %d samples of a gemm-unit\n", stokes_int, samples);
            return EXIT_FAILURE;
        }
    }
    if (select_path.empty() && (!select_ant_path.empty() || !select_chan_path.empty() || sk_sigma_given || sk_centre_given)) {
        fprintf(stderr, "beam: -O / -q / -t / -m belong to the select mode: give -e moments_file\n");
        return EXIT_FAILURE;
    }
    if (!ant_flags_path.empty() && solve_vis.empty() && apply_gains.empty() && null_path.empty()) {
        fprintf(stderr, "beam: -f (antenna flags) belongs to the solvers or to conditioned weights: give -E vis_file, -A gains_file or -Z null_file\n");
        return EXIT_FAILURE;
    }
    if (!select_path.empty()) {   // select mode: host only
        if (observe_mode || !solve_vis.empty() || !apply_gains.empty() || !null_path.empty()) {
            fprintf(stderr, "beam: -e (select flags) runs nothing else: leave out -j / -k / -E / -A / -Z\n");
            return EXIT_FAILURE;
        }
        if (select_ant_path.empty()) {
            fprintf(stderr, "beam: -e needs -O ant_file (where the antenna flags go)\n");
            return EXIT_FAILURE;
        }
        if (select_moments_file(select_path.c_str(), sk_opt, select_ant_path.c_str(), select_chan_path.empty() ? nullptr : select_chan_path.c_str(),
                                std::cout) != BF_OK) {
            fprintf(stderr, "beam: -e %s\n", bf_last_error());
            return EXIT_FAILURE;
        }
        return 0;
    }
    if (!solve_gains_path.empty() && solve_vis.empty()) {
        fprintf(stderr, "beam: -G (where the gains go) belongs to the gain solver: give -E vis_file\n");
        return EXIT_FAILURE;
    }
    if (solve_joint && solve_vis.empty()) {
        fprintf(stderr, "beam: -P (joint polarisations) belongs to the gain solver: give -E vis_file -G gains_file\n");
        return EXIT_FAILURE;
    }
    if (!null_spec.empty()) {   // -y n_null[:min_ratio]: the solver's options
        if (solve_vis.empty() || null_path.empty()) {
            fprintf(stderr, "beam: -y (vectors per channel) belongs to the spatial null's solve mode: give -E vis_file -Z null_file\n");
            return EXIT_FAILURE;
        }
        char* end = nullptr;
        const long n = strtol(null_spec.c_str(), &end, 10);
        double ratio = null_opt.min_ratio;
        bool ok = end != null_spec.c_str() && n >= 1 && n <= BF_NULL_MAX;
        if (ok && *end == ':') {
            char* rend = nullptr;
            ratio = strtod(end + 1, &rend);
            ok = rend != end + 1 && !*rend && ratio >= 0.0;
        } else if (ok && *end) {
            ok = false;
        }
        if (!ok) {
            fprintf(stderr, "beam: -y %s: n_null must be 1 .. %d and min_ratio, if given, a number >= 0\n", null_spec.c_str(), BF_NULL_MAX);
            return EXIT_FAILURE;
        }
        null_opt.n_null = (int)n;
        null_opt.min_ratio = ratio;
    }
    const bool sharded_files = world > 1 && rank >= 0 && rank < world;   // -R: the null's files carry the rank, as -V's do
    if (!solve_vis.empty() && !null_path.empty() && sharded_files) {
        solve_vis += "." + std::to_string(rank);
        null_path += "." + std::to_string(rank);
    }
    std::vector<uint8_t> ant_flags;   // -f: read before any device is touched, against NANT of the vis file (-E) or of the run (-A, -Z)
    if (!solve_vis.empty()) {   // solve mode: no observation of either kind
        if (junk_blocks >= 0 || !ring_key.empty()) {
            fprintf(stderr, "beam: -E (gain solver) runs no observation: leave out -j / -k\n");
            return EXIT_FAILURE;
        }
        if (solve_gains_path.empty() && null_path.empty()) {
            fprintf(stderr, "beam: -E needs -G gains_file (where the gains go) or -Z null_file (where the interferer vectors go)\n");
            return EXIT_FAILURE;
        }
        if (!apply_gains.empty()) {
            fprintf(stderr, "beam: -A (apply gains) belongs to a run; -E only solves\n");
            return EXIT_FAILURE;
        }
        record_file_header vh;
        std::string why;
        if (!read_record_file_header(solve_vis.c_str(), &vh, &why) || vh.content != "visibilities") {
            fprintf(stderr, "beam: -E %s\n", why.empty() ? (solve_vis + " is not a file of visibilities").c_str() : why.c_str());
            return EXIT_FAILURE;
        }
        if (!ant_flags_path.empty() && !read_index_file(ant_flags_path.c_str(), vh.n_ant, &ant_flags, &why)) {
            fprintf(stderr, "beam: -f %s\n", why.c_str());
            return EXIT_FAILURE;
        }
    }
    // -A: read before any device is touched; a DEBUG run has the DEBUG geometry, observation mode a rank's share of the production one
    std::vector<double> gains_layer;
    voltage_file_header coherent_header;   // --coherent: the geometry is the file's; read, with -A and -f, before any device is touched
    if (!coherent_path.empty()) {
        std::string why;
        if (!read_voltage_header(coherent_path.c_str(), &coherent_header, &why)) {
            fprintf(stderr, "beam: --coherent %s\n", why.c_str());
            return EXIT_FAILURE;
        }
        if (!apply_gains.empty() &&
            !read_gains_layer(apply_gains.c_str(), coherent_header.n_ant, coherent_header.n_freq, coherent_header.first_channel, &gains_layer, &why)) {
            fprintf(stderr, "beam: -A %s\n", why.c_str());
            return EXIT_FAILURE;
        }
        if (!ant_flags_path.empty() && !read_index_file(ant_flags_path.c_str(), coherent_header.n_ant, &ant_flags, &why)) {
            fprintf(stderr, "beam: -f %s\n", why.c_str());
            return EXIT_FAILURE;
        }
    }
    if (!apply_gains.empty() && coherent_path.empty()) {
        const bool observe = junk_blocks >= 0 || !ring_key.empty();
        bf_config gcfg;
        bf_config_default(&gcfg, observe ? 0 : 1);
        const int n_freq = observe && world >= 1 && gcfg.n_freq % world == 0 ? gcfg.n_freq / world : gcfg.n_freq;
        const int first = observe && rank >= 0 ? rank * n_freq : 0;
        std::string why;
        if (!read_gains_layer(apply_gains.c_str(), gcfg.n_ant, n_freq, first, &gains_layer, &why)) {
            fprintf(stderr, "beam: -A %s\n", why.c_str());
            return EXIT_FAILURE;
        }
        opt.gains = gains_layer.data();
        if (!ant_flags_path.empty()) {
            if (!read_index_file(ant_flags_path.c_str(), gcfg.n_ant, &ant_flags, &why)) {
                fprintf(stderr, "beam: -f %s\n", why.c_str());
                return EXIT_FAILURE;
            }
            opt.ant_flags = ant_flags.data();
        }
    }
    // -Z without -E: read before any device is touched, against the same geometry as -A
    null_vectors nulls;
    if (!null_path.empty() && solve_vis.empty()) {
        const bool observe = junk_blocks >= 0 || !ring_key.empty();
        bf_config gcfg;
        bf_config_default(&gcfg, observe ? 0 : 1);
        const int n_freq = observe && world >= 1 && gcfg.n_freq % world == 0 ? gcfg.n_freq / world : gcfg.n_freq;
        const int first = observe && rank >= 0 ? rank * n_freq : 0;
        if (observe && sharded_files) null_path += "." + std::to_string(rank);
        std::string why;
        if (!read_null_vectors(null_path.c_str(), gcfg.n_ant, n_freq, first, &nulls, &why)) {
            fprintf(stderr, "beam: -Z %s\n", why.c_str());
            return EXIT_FAILURE;
        }
        opt.nulls = &nulls;
        if (!ant_flags_path.empty() && ant_flags.empty()) {
            if (!read_index_file(ant_flags_path.c_str(), gcfg.n_ant, &ant_flags, &why)) {
                fprintf(stderr, "beam: -f %s\n", why.c_str());
                return EXIT_FAILURE;
            }
        }
        if (!ant_flags.empty()) opt.ant_flags = ant_flags.data();
    }
    opt.positions = positions.empty() ? nullptr : positions.c_str();
    opt.directions = directions.empty() ? nullptr : directions.c_str();
    opt.sources = sources.empty() ? nullptr : sources.c_str();
    opt.output = output.c_str();
    opt.block_launch = !per_unit;

    int n_dev = 0;
    if (bf_device_count(&n_dev) != BF_OK || n_dev == 0) {
        fprintf(stderr, "GPUassert: %s\n", bf_last_error());  // src/beamformer.cuh:26
        return EXIT_FAILURE;
    }
    char name[256];
    if (bf_device_name(opt.device, name, sizeof name) == BF_OK) std::cout << "Selected: " << name << std::endl;

    if (!solve_vis.empty()) {   // -E / -G / -Z: the gain solver and the spatial null on a file of visibilities
        uint64_t n_records = 0;
        if (!solve_gains_path.empty()) {
            int src = solve_vis_file(solve_vis.c_str(), solve_gains_path.c_str(), solve_joint, opt.device, &n_records, std::cout,
                                     ant_flags.empty() ? nullptr : ant_flags.data());
            if (src != BF_OK) {
                fprintf(stderr, "GPUassert: %s (%d)\n", bf_last_error(), src);
                return EXIT_FAILURE;
            }
            std::cout << "Wrote " << n_records << " gain records to " << solve_gains_path << std::endl;
        }
        if (!null_path.empty()) {
            int src = null_vis_file(solve_vis.c_str(), null_path.c_str(), null_opt, opt.device, &n_records, std::cout,
                                    ant_flags.empty() ? nullptr : ant_flags.data());
            if (src != BF_OK) {
                fprintf(stderr, "GPUassert: %s (%d)\n", bf_last_error(), src);
                return EXIT_FAILURE;
            }
            std::cout << "Wrote " << n_records << " null records to " << null_path << std::endl;
        }
        return 0;
    }

    if (!coherent_path.empty()) {   // --coherent: a file of voltage cuts to coherently dedispersed Stokes parameters, no observation
        bf_config pcfg;
        bf_config_default(&pcfg, /*debug=*/0);
        std::vector<antenna> pos((size_t)coherent_header.n_ant);
        std::vector<beam_direction> dir((size_t)pcfg.n_beams);
        if (!opt.positions || read_in_position_locations(opt.positions, coherent_header.n_ant, pos.data()) != 0) default_positions(coherent_header.n_ant, pos.data());
        if (!opt.directions || read_in_beam_directions(opt.directions, pcfg.n_beams, dir.data()) != 0) default_directions(pcfg.n_beams, dir.data());
        coherent_options copt;
        copt.voltages_path = coherent_path.c_str();
        copt.out_path = coherent_out.c_str();
        copt.dm_max = dm_max;
        copt.tsamp_ms = tsamp_ms;
        copt.n_dm_cap = n_dm_cap;
        copt.n_fft = coherent_fft;
        copt.n_int = coherent_int;
        copt.sideband = coherent_sideband;
        copt.gpu = opt.gpu;
        copt.device = opt.device;
        copt.pos = pos.data();
        copt.dir = dir.data();
        copt.gains = gains_layer.empty() ? nullptr : gains_layer.data();
        copt.ant_flags = gains_layer.empty() || ant_flags.empty() ? nullptr : ant_flags.data();
        uint64_t n_written = 0, n_refused = 0;
        const int crc = coherent_voltage_file(copt, &n_written, &n_refused, std::cout);
        if (crc != BF_OK) {
            fprintf(stderr, "GPUassert: %s (%d)\n", bf_last_error(), crc);
            return EXIT_FAILURE;
        }
        std::cout << "Wrote " << n_written << " coherently dedispersed cuts to " << coherent_out << std::endl;
        return 0;
    }

    if (junk_blocks >= 0 || !ring_key.empty()) {  // observation (production) mode: N_AVERAGING 16
        bf_config pcfg;
        bf_config_default(&pcfg, /*debug=*/0);
        pcfg.verbose = cfg.verbose;
        if (world < 1 || rank < 0 || rank >= world || pcfg.n_freq % world) {
            fprintf(stderr, "beam: -R %d -r %d: need 0 <= rank < world and world dividing %d channels\n", world, rank, pcfg.n_freq);
            return EXIT_FAILURE;
        }
        bf_config full_cfg = pcfg;        // the whole sub-band (what the gather root's sink receives)
        pcfg.n_freq /= world;             // this rank's shard
        bf_comm* comm = nullptr;
        if (world > 1 || !id_file.empty()) {
            char id[BF_COMM_ID_BYTES];
            if (id_file.empty()) {
                fprintf(stderr, "beam: -R needs -I idfile (where rank 0 publishes the RCCL unique id)\n");
                return EXIT_FAILURE;
            }
            if (rank == 0) {
                if (bf_comm_unique_id(id) != BF_OK) {
                    fprintf(stderr, "GPUassert: %s\n", bf_last_error());
                    return EXIT_FAILURE;
                }
                // A stale id (a crashed run, a reused name) would make the other ranks join a communicator that no longer
                // exists and hang: rank 0 removes whatever is there, writes a fresh file it alone created (O_EXCL |
                // O_NOFOLLOW: no symlink is followed) and renames it into place -- readers see nothing or the whole id.
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
            } else {
                bool got = false;
                for (int tries = 0; tries < 1200 && !got; tries++) {   // up to 2 minutes
                    std::ifstream in(id_file, std::ios::binary);
                    got = in && in.read(id, sizeof id) && in.gcount() == (std::streamsize)sizeof id;
                    if (!got) std::this_thread::sleep_for(std::chrono::milliseconds(100));
                }
                if (!got) {
                    fprintf(stderr, "beam: rank %d never saw the unique id in %s\n", rank, id_file.c_str());
                    return EXIT_FAILURE;
                }
            }
            if (bf_comm_create(rank, world, id, opt.device, &comm) != BF_OK) {
                fprintf(stderr, "GPUassert: %s\n", bf_last_error());
                return EXIT_FAILURE;
            }
            std::cout << "Shard " << rank << " of " << world << ": channels " << rank * pcfg.n_freq << " .. "
                      << (rank + 1) * pcfg.n_freq - 1 << std::endl;
        }
        std::vector<antenna> pos((size_t)pcfg.n_ant);
        std::vector<beam_direction> dir((size_t)pcfg.n_beams);
        if (!opt.positions || read_in_position_locations(opt.positions, pcfg.n_ant, pos.data()) != 0)
            default_positions(pcfg.n_ant, pos.data());
        if (!opt.directions || read_in_beam_directions(opt.directions, pcfg.n_beams, dir.data()) != 0)
            default_directions(pcfg.n_beams, dir.data());
        std::unique_ptr<block_source> src;
        observation_options oopt;
#ifdef DSABF_WITH_PSRDADA
        unsigned in_key = 0;
        char trailing = 0;
        if (!ring_key.empty() && sscanf(ring_key.c_str(), "%x%c", &in_key, &trailing) == 1) {   // -k baab: src/beamformer.cu:66-75
            char name[] = "beam";
            dada_block_source* s = new dada_block_source(name, core, in_key, std::cout);        // :132
            src.reset(s);
            if (!s->ok()) return EXIT_FAILURE;
            s->expect_block_bytes(bf_bytes_per_block(&pcfg));
            oopt.burn_in = kBurnIn;                                                              // BURNIN reads, :348-355
        } else
#endif
        if (!ring_key.empty()) {  // -k: blocks from the shared-memory ring (the PSRDADA stand-in), no burn-in reads
            shm_block_source* s = new shm_block_source(ring_key.c_str(), core, /*pin=*/true, std::cout);
            src.reset(s);
            if (!s->ok()) return EXIT_FAILURE;  // "Error: could not connect to dada buffer", src/dada_handler.hh:35-38
            s->expect_block_bytes(bf_bytes_per_block(&pcfg));
        } else {                  // -j: the in-memory dada_junkdb source
            junk_block_source* s = new junk_block_source(pcfg, (uint64_t)junk_blocks);
            src.reset(s);
            if (!s->ok()) {
                fprintf(stderr, "beam: could not allocate the junk ring\n");
                return EXIT_FAILURE;
            }
            oopt.burn_in = kBurnIn;
        }
        oopt.gpu = opt.gpu;
        oopt.device = opt.device;
        oopt.verbose = opt.verbose;
        oopt.world = world;
        oopt.rank = rank;
        oopt.comm = comm;
        oopt.incoherent_beam = ib_beam;
        oopt.gains = gains_layer.empty() ? nullptr : gains_layer.data();
        oopt.nulls = opt.nulls;
        oopt.ant_flags = (gains_layer.empty() && !opt.nulls) || ant_flags.empty() ? nullptr : ant_flags.data();
        const bf_config& sink_cfg = comm ? full_cfg : pcfg;
        if (comm && rank != 0) {          // only the gather root has a consumer
            out_ring.clear();
            detected_path.clear();
        }
        std::unique_ptr<detected_sink> sink;
        std::string sink_name;
        if (!out_ring.empty()) {  // -K: hand the detected stream to another process through a shared-memory ring
            ring_sink* rs = new ring_sink(sink_cfg, out_ring.c_str(), 8, opt.gpu);
            sink.reset(rs);
            sink_name = "ring " + out_ring;
            if (!rs->ok() || !rs->is_open()) {
                fprintf(stderr, "beam: could not create ring %s\n", out_ring.c_str());
                return EXIT_FAILURE;
            }
        } else if (!detected_path.empty()) {  // -w: keep the detected stream in a file (the reference drops it, README.md:149)
            file_sink* fs = new file_sink(sink_cfg, detected_path.c_str(), opt.gpu);
            sink.reset(fs);
            sink_name = detected_path;
            if (!fs->ok() || !fs->is_open()) {
                fprintf(stderr, "beam: could not open %s\n", detected_path.c_str());
                return EXIT_FAILURE;
            }
        }
        oopt.sink = sink.get();
        // -M: the DM stage.  Ladder and delay law of sandbox/Dispersion Theory.ipynb (cells 1-2 and 5) over the WHOLE sub-band this
        // run covers (world x n_freq channels), referred to its highest frequency (channel 0): every delay is >= 0.
        std::vector<int32_t> delays;
        std::unique_ptr<dm_file_sink> dm_sink;
        std::unique_ptr<dm_ring_sink> dm_rsink;
        std::unique_ptr<sps_file_sink> cand_sink;
        std::unique_ptr<event_file_sink> esink;
        std::unique_ptr<stamp_file_sink> tsink;
        std::unique_ptr<voltage_file_sink> usink;
        int n_dm = 0, my_trials = 0;
        if (dm_max > 0.0) {
            std::vector<double> dms = dm_trials(0.0, dm_max);
            if (n_dm_cap > 0 && (int)dms.size() > n_dm_cap) {
                std::vector<double> pick;
                for (int i = 0; i < n_dm_cap; i++) pick.push_back(dms[(size_t)((double)i * (dms.size() - 1) / (n_dm_cap > 1 ? n_dm_cap - 1 : 1))]);
                dms.swap(pick);
            }
            n_dm = (int)dms.size();
            std::vector<float> freq((size_t)full_cfg.n_freq);
            for (int c = 0; c < full_cfg.n_freq; c++) freq[(size_t)c] = channel_frequency_weights(opt.gpu, c);
            delays.resize((size_t)n_dm * full_cfg.n_freq);
            dm_delays(dms.data(), n_dm, freq.data(), full_cfg.n_freq, freq[0], tsamp_ms, delays.data());
            int dmax = 0;
            for (int32_t d : delays) dmax = d > dmax ? d : dmax;
            std::cout << "DM stage: " << n_dm << " trials 0 .. " << dms.back() << " pc/cc, largest delay " << dmax << " samples of "
                      << tsamp_ms << " ms" << std::endl;
            oopt.dm_delays = delays.data();
            oopt.n_dm = n_dm;
            int my_first = 0, my_count = n_dm;
            if (dm_split && comm) {       // -X: every rank receives the band and takes its share of the trials
                oopt.gather_root = BF_GATHER_ROOT_ALL;
                oopt.dm_split_trials = true;
                dm_trial_share(n_dm, world, rank, &my_first, &my_count);
                dmax = 0;
                for (size_t i = (size_t)my_first * full_cfg.n_freq; i < (size_t)(my_first + my_count) * full_cfg.n_freq; i++) dmax = delays[i] > dmax ? delays[i] : dmax;
                if (!dm_path.empty()) dm_path += "." + std::to_string(rank);
                if (!cand_path.empty()) cand_path += "." + std::to_string(rank);
                if (!events_path.empty()) events_path += "." + std::to_string(rank);
                if (!stamps_path.empty()) stamps_path += "." + std::to_string(rank);
                std::cout << "Shard " << rank << " dedisperses trials " << my_first << " .. " << my_first + my_count - 1 << std::endl;
            }
            my_trials = my_count;
            if (!dm_path.empty() && my_count > 0 && (!comm || rank == 0 || oopt.dm_split_trials)) {
                dm_sink.reset(new dm_file_sink(pcfg, full_cfg.n_freq, my_count, dmax, dm_path.c_str(), opt.gpu, my_first));
                if (!dm_sink->is_open()) {
                    fprintf(stderr, "beam: could not open %s\n", dm_path.c_str());
                    return EXIT_FAILURE;
                }
                oopt.dm_sink = dm_sink.get();
            } else if (!dm_ring.empty() && my_count > 0 && (!comm || rank == 0 || oopt.dm_split_trials)) {
                // -Q: hand the chunks to another process (the downstream search) through a shared-memory ring
                if (oopt.dm_split_trials) dm_ring += "." + std::to_string(rank);
                dm_rsink.reset(new dm_ring_sink(pcfg, full_cfg.n_freq, my_count, dmax, pcfg.n_gemms_per_block * pcfg.n_out_per_gemm,
                                                dm_ring.c_str(), 4, opt.gpu, my_first));
                if (!dm_rsink->is_open()) {
                    fprintf(stderr, "beam: could not create ring %s\n", dm_ring.c_str());
                    return EXIT_FAILURE;
                }
                oopt.dm_sink = dm_rsink.get();
            }
        }
        if (sps_on && my_trials > 0 && (!comm || rank == 0 || oopt.dm_split_trials)) {   // -S: the search runs where the DM stage runs
            oopt.sps_widths = sps_widths;
            oopt.sps_threshold = sps_snr;
            if (!cand_path.empty()) {
                cand_sink.reset(new sps_file_sink(cand_path.c_str()));
                if (!cand_sink->is_open()) {
                    fprintf(stderr, "beam: could not open %s\n", cand_path.c_str());
                    return EXIT_FAILURE;
                }
                oopt.sps_sink = cand_sink.get();
            }
            if (!events_path.empty()) {   // --events / --stamps: where the search runs
                esink.reset(new event_file_sink(events_path.c_str()));
                if (!esink->is_open()) {
                    fprintf(stderr, "beam: could not open %s\n", events_path.c_str());
                    return EXIT_FAILURE;
                }
                oopt.evt = &evt_opt;
                oopt.event_sink = esink.get();
                oopt.stamp_bins = stamp_bins;
                oopt.stamp_tbin = stamp_tbin;
                oopt.stamp_fbin = stamp_fbin;
                oopt.stamp_flagged = stamp_flagged;
                if (!stamps_path.empty()) {
                    tsink.reset(new stamp_file_sink(stamps_path.c_str(), full_cfg.n_freq / stamp_fbin, stamp_bins, stamp_fbin));
                    if (!tsink->is_open()) {
                        fprintf(stderr, "beam: could not open %s\n", stamps_path.c_str());
                        return EXIT_FAILURE;
                    }
                    oopt.stamp_sink = tsink.get();
                }
                if (!voltages_path.empty()) {
                    usink.reset(new voltage_file_sink(voltages_path.c_str(), pcfg, voltage_units, 0));
                    if (!usink->is_open()) {
                        fprintf(stderr, "beam: could not open %s\n", voltages_path.c_str());
                        return EXIT_FAILURE;
                    }
                    oopt.vcut_sink = usink.get();
                    oopt.vcut_units = voltage_units;
                    oopt.vcut_history_units = voltage_history;
                    oopt.vcut_flagged = voltage_flagged;
                }
            }
        }
        if (cond_given && my_trials > 0 && (!comm || rank == 0 || oopt.dm_split_trials)) {   // -n: the conditioner runs where the DM stage runs
            oopt.cond_baseline = cond_n;
            oopt.cond_zero_dm = cond_zdm;
            oopt.cond_auto_threshold = cond_auto;
            if (!cond_mask.empty() && (int)cond_mask.size() != full_cfg.n_freq) {   // (-F was checked against the production band)
                fprintf(stderr, "beam: -F: the mask has %zu channels, the band of this run %d\n", cond_mask.size(), full_cfg.n_freq);
                return EXIT_FAILURE;
            }
            oopt.cond_mask = cond_mask.empty() ? nullptr : cond_mask.data();
        }
        std::vector<bf_psr_model> fold_models;
        std::vector<int32_t> fold_delays;
        std::unique_ptr<psr_file_sink> fsink;
        if (!folds.empty() && my_trials > 0 && (!comm || rank == 0 || oopt.dm_split_trials)) {   // --fold: the folder runs where the DM stage runs
            const int n_psr = (int)folds.size();
            std::vector<double> dms((size_t)n_psr, 0.0);
            for (size_t k = 0; k < fold_dms.size(); k++) dms[k] = fold_dms[k];
            std::vector<float> freq((size_t)full_cfg.n_freq);
            for (int c = 0; c < full_cfg.n_freq; c++) freq[(size_t)c] = channel_frequency_weights(opt.gpu, c);
            fold_delays.resize((size_t)n_psr * full_cfg.n_freq);
            dm_delays(dms.data(), n_psr, freq.data(), full_cfg.n_freq, freq[0], tsamp_ms, fold_delays.data());
            fold_models.resize((size_t)n_psr);
            for (int k = 0; k < n_psr; k++)
                if (bf_psr_model_from_spin(folds[(size_t)k].f0, folds[(size_t)k].f1, folds[(size_t)k].phase0, tsamp_ms * 1e-3, 0, &fold_models[(size_t)k]) != BF_OK) {
                    fprintf(stderr, "beam: --fold %d: %s\n", k, bf_last_error());
                    return EXIT_FAILURE;
                }
            oopt.psr_models = fold_models.data();
            oopt.psr_delays = fold_delays.data();
            oopt.n_psr = n_psr;
            oopt.psr_bins = fold_bins;
            oopt.psr_dump_rows = fold_rows > 0 ? fold_rows : pcfg.n_gemms_per_block * pcfg.n_out_per_gemm;
            if (!fold_path.empty()) {
                if (oopt.dm_split_trials) fold_path += "." + std::to_string(rank);
                fsink.reset(new psr_file_sink(fold_path.c_str(), n_psr, full_cfg.n_freq, fold_bins, pcfg.n_beams));
                if (!fsink->is_open()) {
                    fprintf(stderr, "beam: could not open %s\n", fold_path.c_str());
                    return EXIT_FAILURE;
                }
                oopt.psr_sink = fsink.get();
            }
            std::cout << "Pulsar folder: " << n_psr << " pulsars, " << fold_bins << " bins, a dump every " << oopt.psr_dump_rows << " rows of " << tsamp_ms
                      << " ms" << std::endl;
        }
        inj_plan iplan;
        if (inj_given && my_trials > 0 && (!comm || rank == 0 || oopt.dm_split_trials)) {   // --inject: the injector runs where the DM stage runs
            const int n_f = full_cfg.n_freq, n_b = pcfg.n_beams;
            std::vector<float> freq((size_t)n_f);
            for (int c = 0; c < n_f; c++) freq[(size_t)c] = channel_frequency_weights(opt.gpu, c);
            FILE* truth = nullptr;
            if (!inj_path.empty()) {
                if (oopt.dm_split_trials) inj_path += "." + std::to_string(rank);
                truth = fopen(inj_path.c_str(), "w");
                if (!truth) {
                    fprintf(stderr, "beam: could not open %s\n", inj_path.c_str());
                    return EXIT_FAILURE;
                }
                fprintf(truth, "# id kind t0|f0 dm trial beam fluence|amp sigma|duty w|bins [t_lo t_hi]\n");
            }
            // delays of one pulse at the run's channel frequencies and -T, as --fold-dm takes them; its nearest trial of the whole ladder
            auto delays_of = [&](double dm, std::vector<int32_t>* d, int* trial) {
                d->resize((size_t)n_f);
                dm_delays(&dm, 1, freq.data(), n_f, freq[0], tsamp_ms, d->data());
                return bf_inj_nearest_trial(delays.data(), n_dm, n_f, d->data(), trial);
            };
            bool ok = true;
            uint64_t id = 0;
            for (const inject_spec& sp : inj_bursts) {
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
                iplan.bursts.push_back(std::move(b));
            }
            for (const inject_spec& sp : inj_trains) {
                inj_plan::train t;
                int trial = -1;
                t.n_bins = (int)sp.v[5];
                ok = ok && sp.v[2] < n_b && delays_of(sp.v[1], &t.delay, &trial) == BF_OK;
                ok = ok && bf_psr_model_from_spin(sp.v[0], 0.0, 0.0, tsamp_ms * 1e-3, 0, &t.model) == BF_OK;
                const int on = std::max(1, (int)std::lround(sp.v[4] * t.n_bins));
                t.profile.assign((size_t)n_f * (size_t)t.n_bins, 0.0f);
                for (int f = 0; f < n_f; f++)
                    for (int j = 0; j < on; j++) t.profile[(size_t)f * (size_t)t.n_bins + (size_t)j] = (float)sp.v[3];
                t.response.assign((size_t)n_b, 0.0f);
                if (ok) t.response[(size_t)sp.v[2]] = 1.0f;
                if (ok && truth)
                    fprintf(truth, "%llu train %.17g %.17g %d %d %.17g %.17g %d\n", (unsigned long long)id, sp.v[0], sp.v[1], trial, (int)sp.v[2], sp.v[3], sp.v[4],
                            t.n_bins);
                id++;
                iplan.trains.push_back(std::move(t));
            }
            if (truth) fclose(truth);
            if (!ok) {
                fprintf(stderr, "beam: --inject / --inject-train: BEAM must be below the %d beams of this run, and the pulse must fit its window (%s)\n", n_b,
                        bf_last_error());
                return EXIT_FAILURE;
            }
            oopt.inj = &iplan;
            std::cout << "Injector: " << iplan.bursts.size() << " bursts and " << iplan.trains.size() << " trains in front of the DM stage" << std::endl;
        }
        std::unique_ptr<ffa_file_sink> ffa_out;
        if (ffa_given && my_trials > 0 && (!comm || rank == 0 || oopt.dm_split_trials)) {   // --ffa: the search runs where the DM stage runs
            oopt.ffa_p_lo = ffa_p_lo;
            oopt.ffa_p_hi = ffa_p_hi;
            oopt.ffa_seg = ffa_seg;
            oopt.ffa_dec = ffa_dec;
            oopt.ffa_oct = ffa_oct;
            oopt.ffa_widths = ffa_widths;
            oopt.ffa_threshold = ffa_snr;
            oopt.ffa_detrend_blk = ffa_det_blk;
            oopt.ffa_detrend_win = ffa_det_win;
            if (!ffa_path.empty()) {
                if (oopt.dm_split_trials) ffa_path += "." + std::to_string(rank);   // one file per shard; the trials are numbered over the whole ladder
                ffa_out.reset(new ffa_file_sink(ffa_path.c_str(), ffa_dec, ffa_seg, ffa_oct, ffa_p_lo, ffa_p_hi, ffa_widths, ffa_snr, ffa_det_blk, ffa_det_win));
                if (!ffa_out->is_open()) {
                    fprintf(stderr, "beam: could not open %s\n", ffa_path.c_str());
                    return EXIT_FAILURE;
                }
                oopt.ffa_sink = ffa_out.get();
            }
        }
        std::unique_ptr<vis_file_sink> vsink;
        if (!vis_path.empty()) {   // -V: every shard correlates its own channels
            if (comm) vis_path += "." + std::to_string(rank);
            vsink.reset(new vis_file_sink(pcfg, vis_path.c_str(), rank * pcfg.n_freq, opt.gpu));
            if (!vsink->is_open()) {
                fprintf(stderr, "beam: could not open %s\n", vis_path.c_str());
                return EXIT_FAILURE;
            }
            oopt.corr_blocks = corr_blocks;
            oopt.vis_sink = vsink.get();
        }
        std::unique_ptr<sk_file_sink> ksink;
        if (!sk_path.empty()) {   // -Y: every shard measures its own channels
            if (comm) sk_path += "." + std::to_string(rank);
            ksink.reset(new sk_file_sink(pcfg, sk_path.c_str(), rank * pcfg.n_freq, opt.gpu));
            if (!ksink->is_open()) {
                fprintf(stderr, "beam: could not open %s\n", sk_path.c_str());
                return EXIT_FAILURE;
            }
            oopt.sk_blocks = sk_blocks;
            oopt.sk_sink = ksink.get();
        }
        std::unique_ptr<stokes_file_sink> xsink;
        if (!stokes_path.empty()) {   // -x: every shard follows the beams in its own channels
            if (comm) stokes_path += "." + std::to_string(rank);
            const int n_int = stokes_int_given ? stokes_int : pcfg.n_avg;
            xsink.reset(new stokes_file_sink(pcfg, stokes_path.c_str(), rank * pcfg.n_freq, opt.gpu, stokes_beams, n_int));
            if (!xsink->is_open()) {
                fprintf(stderr, "beam: could not open %s\n", stokes_path.c_str());
                return EXIT_FAILURE;
            }
            oopt.stokes_beams = stokes_beams;
            oopt.stokes_int = n_int;
            oopt.stokes_sink = xsink.get();
        }
        observation_result ores;
        int orc = run_observation(pcfg, oopt, *src, pos.data(), dir.data(), &ores, std::cout);
        if (sink) std::cout << "Wrote " << sink->get_delivered() << " gemm-units of detected powers to " << sink_name << std::endl;
        if (dm_sink) std::cout << "Wrote " << dm_sink->get_times_written() << " dedispersed samples x " << my_trials << " trials to " << dm_path << std::endl;
        if (cand_sink) std::cout << "Wrote " << cand_sink->get_candidates_written() << " candidates to " << cand_path << std::endl;
        if (ffa_out) std::cout << "Wrote " << ffa_out->get_candidates_written() << " periodicity candidates to " << ffa_path << std::endl;
        if (esink) std::cout << "Wrote " << esink->get_events_written() << " events to " << events_path << std::endl;
        if (tsink) std::cout << "Wrote " << tsink->get_stamps_written() << " stamps to " << stamps_path << std::endl;
        if (usink) std::cout << "Wrote " << usink->get_cuts_written() << " voltage cuts to " << voltages_path << std::endl;
        if (vsink) std::cout << "Wrote " << vsink->get_dumps_written() << " visibility dumps of " << corr_blocks << " blocks to " << vis_path << std::endl;
        if (xsink) std::cout << "Wrote " << xsink->get_sets_written() << " sets of Stokes beams to " << stokes_path << std::endl;
        if (ksink) std::cout << "Wrote " << ksink->get_dumps_written() << " moment dumps of " << sk_blocks << " blocks to " << sk_path << std::endl;
        bf_comm_destroy(comm);
        if (orc != BF_OK) {
            fprintf(stderr, "GPUassert: %s (%d)\n", bf_last_error(), orc);
            return EXIT_FAILURE;
        }
        return 0;
    }

    debug_run_result res;
    int rc = run_debug_observation(cfg, opt, &res, nullptr, std::cout);
    if (rc != BF_OK) {
        fprintf(stderr, "GPUassert: %s (%d)\n", bf_last_error(), rc);
        return EXIT_FAILURE;  // the reference exit()s inside gpuErrchk; the driver keeps that policy here
    }
    std::cout << "Freeing CUDA Structures" << std::endl;
    std::cout << "Freed GPU memory" << std::endl;
    std::cout << "Freed CPU memory" << std::endl;
    return 0;
}
