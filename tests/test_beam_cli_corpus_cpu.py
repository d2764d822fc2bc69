"""The `beam` driver's command line against a recorded corpus (csrc/beam_main.cpp): every refusal that is printed before a device is
touched, pairs of faults that pin the order of neighbouring checks, both sides of every numeric field's boundaries, and the file-level
refusals of -e / -E / -A / -Z / -f / --coherent / -F.  tests/golden/beam_cli_corpus.json holds, per command line, the exit status,
stdout, stderr and the files the run left in its working directory; a restructured driver has to reproduce all of it exactly.

A record with "device": true is a command line that passes every check and reaches the device: without a GPU it ends in
`GPUassert: ...`, and only that class is asserted (with a GPU it would start a run, so it is left out there).

    python tests/test_beam_cli_corpus_cpu.py path/to/beam      writes the fixture from that binary
"""
import json
import os
import struct
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "beam_cli_corpus.json")
T = "{tmp}/"


def _header(**kv):
    text = "".join("%s %s\n" % (k, v) for k, v in kv.items()).encode()
    return text + b"\0" * (4096 - len(text))


def _record_header(content, dtype, n_freq, first, **more):
    return _header(HDR_SIZE=4096, CONTENT=content, DTYPE=dtype, RECORD_HEADER_BYTES=16, NANT=64, NPOL=1, NFREQ=n_freq, FIRST_CHANNEL=first, **more)


def make_inputs(tmp):
    """The small input files some command lines need."""
    def put(name, data, size=None):
        with open(os.path.join(tmp, name), "wb") as fp:
            fp.write(data)
            if size is not None:
                fp.truncate(size)   # (zeros, sparse)

    put("idx_ok", b"# flagged\n3\n 5 # five\n\n7\t\n")
    put("idx_range", b"3\n9999\n")
    put("idx_neg", b"-1\n")
    put("idx_junk", b"3\nabc\n")
    put("short", b"too short for a header\n")
    put("vis_ok", _header(HDR_SIZE=4096, CONTENT="visibilities", DTYPE="int64", RECORD_HEADER_BYTES=16, NANT=64, NPOL=2, NFREQ=256, FIRST_CHANNEL=0))
    put("vis_ok.1", _header(HDR_SIZE=4096, CONTENT="visibilities", DTYPE="int64", RECORD_HEADER_BYTES=16, NANT=64, NPOL=2, NFREQ=128, FIRST_CHANNEL=128))
    put("vis_wrong", _record_header("gains", "float64", 256, 0))
    put("vis_nokey", _header(HDR_SIZE=4096, CONTENT="visibilities"))
    put("volt_ok", _header(HDR_SIZE=4096, CONTENT="voltages", DTYPE="packed4+4", RECORD_HEADER_BYTES=28, NANT=64, NPOL=2, NFREQ=256, NAVG=16, NOUT=8, UNITS=2,
                           FIRST_CHANNEL=0))
    put("volt_wrong", _header(HDR_SIZE=4096, CONTENT="voltages", DTYPE="int8", RECORD_HEADER_BYTES=28, NANT=64, NPOL=2, NFREQ=256, NAVG=16, NOUT=8, UNITS=2,
                              FIRST_CHANNEL=0))
    # one record of gains: 16 bytes, [pol][freq][ant]{re, im} float64, [pol][freq]{iterations, converged} int32
    for name, n_freq, first in (("gains_full", 256, 0), ("gains_shard", 64, 64)):
        put(name, _record_header("gains", "float64", n_freq, first), 4096 + 16 + n_freq * 64 * 16 + n_freq * 8)
    put("gains_empty", _record_header("gains", "float64", 256, 0))
    # one record of interferer vectors: 16 bytes, vectors, eigenvalues, info
    for name, n_freq, first in (("null_full", 256, 0), ("null_shard.1", 64, 64)):
        put(name, _record_header("nullvecs", "float64", n_freq, first, NNULL=1), 4096 + 16 + n_freq * 64 * 16 + n_freq * 2 * 8 + n_freq * 3 * 4)
    put("null_nonull", _record_header("nullvecs", "float64", 256, 0))
    # two records of voltage moments of 2 channels x 2 polarisations x 4 antennas, 1024 columns each: sum |v|^2 = 1024 m, sum |v|^4 = 2048 m^2
    # (a complex Gaussian), antenna 2 of the first channel with a fourth moment three times that
    moments = []
    for i in range(2 * 2 * 4):
        m = 10 + i
        moments += [1024 * m, 2048 * m * m * (3 if i == 2 else 1)]
    rec = struct.pack("<2Q", 0, 1024) + struct.pack("<%dq" % len(moments), *moments)
    put("moments_ok", _header(HDR_SIZE=4096, CONTENT="voltage_moments", DTYPE="int64", RECORD_HEADER_BYTES=16, NANT=4, NPOL=2, NFREQ=2, FIRST_CHANNEL=6) + rec + rec)


DM = ["-M", "40"]
SPS = DM + ["-S", "8"]
EV = SPS + ["--events", "e"]
ST = EV + ["--stamps", "s"]
VO = EV + ["--voltages", "v"]
OBS = ["-j", "27"]
CO = ["--coherent", T + "volt_ok", "--coherent-out", "o"] + DM
NUL = ["-E", T + "vis_ok", "-Z", "n"]
FOLD = DM + ["--fold", "3.3"]
FFA = DM + ["--ffa", "8:13"]


def corpus():
    c = []

    def each(prefix, option, values):
        c.extend(prefix + [option, v] for v in values)

    # the texts, the reference's exits
    c += [[], ["-h"], ["-H"], ["--bogus"], ["-9"], ["-M"], ["--event", "e"], ["--stamp-f"], ["--fold-b", "16"], ["-h", "-S", "8"], ["-S", "8", "-H"], ["--bogus", "-h"]]
    # every refusal in front of the device, in the order of the checks (several lines each where a rule has several triggers)
    c += [["-S", "8"], ["-S", "8", "-M", "0"], ["-S", "8", "-M", "nan"], ["-B", "3"], ["-C", "c"], DM + ["-B", "3", "-C", "c"],
          ["--fold", "3.3"], DM + ["--fold-dm", "20"], DM + ["--fold-bins", "16"], DM + ["--fold-rows", "64"], DM + ["--fold-out", "x"],
          DM + ["--fold", "1", "--fold", "2", "--fold", "3", "--fold", "4", "--fold", "5"], DM + ["--fold", "1", "--fold", "2", "--fold", "3", "--fold", "4"],
          FOLD + ["--fold-dm", "1", "--fold-dm", "2"], DM + ["--fold", "1", "--fold-dm", "1", "--fold", "2", "--fold-dm", "2"],
          ["--inject", "300:20:3:6"], ["--inject-train", "3.3:20:3:0.5"], ["--inject-out", "x"],
          OBS + ["--inject", "300:20:3:6:1.5:16", "--inject-train", "3.3:20:3:0.5:0.1:32", "--inject-out", "x"], DM + ["--inject-out", "x"],
          DM + sum((["--inject-train", "%d:20:3:0.5" % (1 + k)] for k in range(5)), []), DM + sum((["--inject-train", "%d:20:3:0.5" % (1 + k)] for k in range(4)), []),
          ["--ffa", "8:13"], OBS + ["--ffa", "64:128", "--ffa-seg", "8192", "--ffa-out", "x"]]
    each(DM, "--ffa-seg", ["64"]), each(DM, "--ffa-dec", ["2"]), each(DM, "--ffa-oct", ["2"]), each(DM, "--ffa-widths", ["2"]), each(DM, "--ffa-snr", ["7"])
    each(DM, "--ffa-out", ["x"]), each(DM, "--ffa-detrend", ["4:9"])
    c += [["--events", "e"], DM + ["--events", "e"], ["--event-tol", "3"], ["--event-veto", "4"], ["--stamps", "s"], SPS + ["--stamps", "s"],
          ["--stamp-shape", "64"], ["--stamp-flagged"], EV + ["--stamp-flagged"],
          ["--voltage-units", "2"], ["--voltage-history", "8"], ["--voltage-flagged"], ["--voltages", "v"], SPS + ["--voltages", "v"], VO + ["-R", "2"],
          VO + ["-R", "1"], VO, VO + ["--voltage-units", "3", "--voltage-history", "9", "--voltage-flagged"],
          ["--coherent-out", "o"], ["--coherent-fft", "64"], ["--coherent-int", "2"], ["--coherent-sideband", "-1"],
          CO + OBS, CO + ["-k", "ring"], CO + ["-E", T + "vis_ok"], ["--coherent", T + "volt_ok"] + DM, ["--coherent", T + "volt_ok", "--coherent-out", "o"],
          CO + ["-T", "0"], CO + ["-T", "-1"], CO + ["-T", "nan"], CO + ["-T", "0.131", "-N", "4"],
          ST + ["--stamp-shape", "64:0:7"], SPS + ["-B", "0"], SPS + ["-B", "9"], SPS + ["-B", "1"], SPS + ["-B", "8"], SPS + ["-B", "x"],
          ["-n", "4"], ["-z"], ["-U", "3"], ["-F", T + "idx_ok"], DM + ["-z"], DM + ["-U", "3"], DM + ["-F", T + "idx_ok"],
          DM + ["-n", "0"], DM + ["-n", "65"], DM + ["-n", "1"], DM + ["-n", "64", "-z"], DM + ["-n", "x"], DM + ["-n", "4", "-U", "-1"], DM + ["-n", "4", "-U", "nan"],
          DM + ["-n", "4", "-U", "0"], DM + ["-n", "4", "-F", T + "missing"], DM + ["-n", "4", "-F", T + "idx_junk"], DM + ["-n", "4", "-F", T + "idx_range"],
          DM + ["-n", "4", "-F", T + "idx_neg"], DM + ["-n", "4", "-F", T + "idx_ok"], DM + ["-n", "4", "-F", T + "short"],
          ["-i", "9999"], ["-i", "-1"], ["-i", "256"], ["-i", "255"], ["-i", "3"], OBS + ["-i", "0"], ["-k", "ring", "-i", "255"],
          ["-L", "2"], ["-V", "v", "-L", "0"], ["-V", "v"], ["-V", "v", "-L", "1"], OBS + ["-V", "v", "-L", "2"],
          ["-J", "2"], ["-Y", "y", "-J", "0"], ["-Y", "y"], OBS + ["-Y", "y", "-J", "2"],
          ["-b", "1"], ["-l", "4"], ["-x", "s"], ["-x", "s", "-b", "1"], OBS + ["-x", "s"], OBS + ["-x", "s", "-b", "999"], OBS + ["-x", "s", "-b", "1,x"],
          OBS + ["-x", "s", "-b", "1,1"], OBS + ["-x", "s", "-b", "1,"], OBS + ["-x", "s", "-b", ",".join(str(k) for k in range(17))],
          OBS + ["-x", "s", "-b", ",".join(str(k) for k in range(16))], OBS + ["-x", "s", "-b", "1,2", "-l", "0"], OBS + ["-x", "s", "-b", "1,2", "-l", "3"],
          OBS + ["-x", "s", "-b", "1,2", "-l", "129"], OBS + ["-x", "s", "-b", "1,2", "-l", "128"], OBS + ["-x", "s", "-b", "1,2", "-l", "1"],
          ["-O", "a"], ["-q", "q"], ["-t", "5"], ["-m", "1"], ["-f", T + "idx_ok"],
          ["-e", T + "moments_ok"] + OBS, ["-e", T + "moments_ok", "-k", "r"], ["-e", T + "moments_ok", "-E", "v"], ["-e", T + "moments_ok", "-A", "g"],
          ["-e", T + "moments_ok", "-Z", "n"], ["-e", T + "moments_ok"], ["-e", T + "missing", "-O", "a"], ["-e", T + "short", "-O", "a"],
          ["-e", T + "vis_ok", "-O", "a"], ["-e", T + "moments_ok", "-O", "a"], ["-e", T + "moments_ok", "-O", "a", "-q", "q", "-t", "3", "-m", "1.5"],
          ["-e", T + "moments_ok", "-O", "a", "-S", "8"], ["-e", T + "moments_ok", "-O", "a", "-G", "g", "-P", "-y", "2"],
          ["-G", "g"], ["-P"], ["-y", "2"], ["-E", "v", "-y", "2"], ["-Z", "n", "-y", "2"],
          ["-E", T + "vis_ok"] + OBS, ["-E", T + "vis_ok", "-k", "r"], ["-E", T + "vis_ok"], ["-E", T + "vis_ok", "-G", "g", "-A", "a"],
          ["-E", T + "missing", "-G", "g"], ["-E", T + "short", "-G", "g"], ["-E", T + "vis_wrong", "-G", "g"], ["-E", T + "vis_nokey", "-Z", "n"],
          ["-E", T + "vis_ok", "-G", "g"], ["-E", T + "vis_ok", "-G", "g", "-P", "-f", T + "idx_ok"], ["-E", T + "vis_ok", "-G", "g", "-f", T + "idx_range"],
          ["-E", T + "vis_ok", "-G", "g", "-f", T + "idx_junk"], ["-E", T + "vis_ok", "-Z", "n", "-f", T + "missing"], NUL, NUL + ["-G", "g"],
          NUL + ["-R", "2", "-r", "1"], ["-E", T + "missing", "-Z", "n", "-R", "2", "-r", "1"], ["-E", T + "missing", "-Z", "n", "-R", "2", "-r", "2"],
          ["-E", T + "missing", "-G", "g", "-R", "2", "-r", "1"],
          ["--coherent", T + "missing", "--coherent-out", "o"] + DM, ["--coherent", T + "short", "--coherent-out", "o"] + DM,
          ["--coherent", T + "volt_wrong", "--coherent-out", "o"] + DM, CO, CO + ["-A", T + "missing"], CO + ["-A", T + "gains_shard"], CO + ["-A", T + "gains_full"],
          CO + ["-f", T + "idx_junk"], CO + ["-A", T + "gains_full", "-f", T + "idx_range"], CO + ["-A", T + "gains_full", "-f", T + "idx_ok"],
          CO + ["-Z", T + "null_full"], CO + ["-Z", T + "missing"],
          ["-A", T + "missing"], ["-A", T + "short"], ["-A", T + "vis_ok"], ["-A", T + "gains_empty"], ["-A", T + "gains_shard"], ["-A", T + "gains_full"],
          OBS + ["-A", T + "gains_full"], OBS + ["-A", T + "gains_shard"], OBS + ["-R", "4", "-r", "1", "-A", T + "gains_shard"],
          OBS + ["-R", "4", "-r", "1", "-A", T + "gains_full"], OBS + ["-R", "3", "-r", "1", "-A", T + "gains_full"], OBS + ["-R", "4", "-r", "-1", "-A", T + "gains_shard"],
          OBS + ["-R", "0", "-r", "1", "-A", T + "gains_shard"], ["-R", "4", "-r", "1", "-A", T + "gains_full"], ["-k", "r", "-R", "4", "-r", "1", "-A", T + "gains_full"],
          ["-A", T + "gains_full", "-f", T + "idx_junk"], ["-A", T + "gains_full", "-f", T + "missing"], ["-A", T + "gains_full", "-f", T + "idx_ok"],
          ["-Z", T + "missing"], ["-Z", T + "short"], ["-Z", T + "gains_full"], ["-Z", T + "null_nonull"], ["-Z", T + "null_full"], OBS + ["-Z", T + "null_full"],
          OBS + ["-R", "4", "-r", "1", "-Z", T + "null_shard"], OBS + ["-R", "4", "-r", "1", "-Z", T + "null_full"], OBS + ["-R", "4", "-r", "5", "-Z", T + "null_full"],
          ["-R", "4", "-r", "1", "-Z", T + "null_full"], OBS + ["-R", "3", "-r", "1", "-Z", T + "null_full"],
          ["-Z", T + "null_full", "-f", T + "idx_range"], ["-Z", T + "null_full", "-f", T + "idx_ok"],
          ["-A", T + "gains_full", "-Z", T + "null_full", "-f", T + "idx_ok"], ["-A", T + "gains_full", "-Z", T + "null_full", "-f", T + "idx_junk"],
          ["-A", T + "gains_full", "-Z", T + "missing"]]
    # pairs of faults: the earlier check speaks
    c += [["-S", "8", "-B", "3", "--fold", "3.3"], DM + ["-S", "8", "-B", "9", "-n", "99"], OBS + DM + ["-i", "9999", "-L", "0"],
          ["-B", "3", "--fold", "3.3"], ["--fold", "abc"], DM + ["--fold-bins", "16x"], DM + ["--fold", "abc", "--inject-out", "x"], DM + ["--fold", "abc", "--inject", "abc"],
          ["--fold-dm", "x", "--inject", "300:20:3:6"], ["--inject", "abc"], DM + ["--inject-out", "x", "--ffa-seg", "64"], DM + ["--inject", "abc", "--ffa-seg", "64"],
          ["--inject", "300:20:3:6", "--ffa", "8:13"], ["--ffa", "8"], DM + ["--ffa-seg", "64k"], DM + ["--ffa", "8", "--event-tol", "-3"],
          ["--event-tol", "x", "--events", "e"], ["--events", "e", "--stamp-flagged"], ["--event-tol", "3", "--stamp-flagged"], ["--stamp-flagged", "--voltage-units", "0"],
          ["--voltage-units", "0"], ["--voltage-flagged", "--coherent-out", "o"], ["--voltages", "v", "-R", "2"], VO + ["-R", "2", "--coherent-fft", "64"],
          SPS + ["-B", "9", "--coherent-int", "2"], ["--coherent", "v"] + OBS, ["--coherent", "v"], ["--coherent", "v", "--coherent-out", "o", "--coherent-fft", "100"],
          ["--coherent", "v", "--coherent-out", "o", "--coherent-fft", "100", "-T", "0"] + DM, ["--coherent", "v", "--coherent-out", "o", "-T", "0", "-S", "8", "-B", "9"] + DM,
          ST + ["--stamp-shape", "64:0:7", "-B", "9"], SPS + ["-B", "9", "-z"], DM + ["-n", "0", "-U", "-1"], DM + ["-n", "4", "-U", "-1", "-F", T + "missing"],
          DM + ["-n", "4", "-F", T + "missing", "-i", "9999"], DM + ["-n", "4", "-F", T + "idx_junk", "-i", "9999"], ["-i", "3", "-L", "2"], ["-L", "0"],
          ["-V", "v", "-J", "2"], ["-J", "0"], ["-Y", "y", "-J", "0", "-b", "1"], ["-Y", "y", "-b", "1"], ["-b", "1", "-O", "a"], ["-x", "s", "-O", "a"],
          OBS + ["-x", "s", "-l", "0"], OBS + ["-x", "s", "-b", "999", "-l", "0"], OBS + ["-x", "s", "-b", "1,2", "-l", "3", "-O", "a"], ["-O", "a", "-f", "f"],
          ["-f", "f", "-G", "g"], ["-e", "m"] + OBS, ["-e", T + "missing"], ["-e", T + "missing", "-O", "a", "-G", "g"], ["-G", "g", "-P"], ["-P", "-y", "2"],
          ["-y", "2", "-E", "v"] + OBS, ["-E", "v", "-Z", "n", "-y", "0"] + OBS, ["-E", "v", "-A", "g"] + OBS, ["-E", "v", "-A", "g"],
          ["-E", T + "missing", "-G", "g", "-A", "a"], ["-E", T + "missing", "-G", "g", "-f", T + "idx_junk"],
          ["-E", T + "vis_ok", "-G", "g", "-f", T + "idx_junk", "--coherent", T + "missing"], ["-A", T + "missing", "-Z", T + "missing"],
          ["-A", T + "missing", "-f", T + "idx_junk"], ["-Z", T + "missing", "-f", T + "idx_junk"], ["-A", T + "gains_full", "-f", T + "idx_junk", "-Z", T + "missing"],
          CO + ["-A", T + "missing", "-f", T + "idx_junk"], OBS + ["-R", "2", "-r", "5", "-A", T + "missing"], DM + ["-n", "4", "-F", T + "missing", "-A", T + "missing"]]
    # numeric fields: both sides of every boundary, every forbidden leading character
    each(EV, "--event-tol", ["3", "3,2", "0", "0,0", "+3", " 3", "\t3", "-3", "3x", "", "3,", "3,2,1", "3:2", "1000000000", "1000000001", ",2", "3,+2", "3,-2", "3, 2", "3,2x"])
    each(EV, "--event-veto", ["4", "4:0.5", "4:", "4:x", "4:-1", "4:0", "4:nan", "4:inf", "4:0.5x", "+4", "-4", " 4", "", "4:0.5:1", "4: 0.5", "4:+0.5", "4,0.5", "1000000001"])
    each(ST, "--stamp-shape", ["64", "64:0", "64:0:1", "64:0:1:2", "0", "1", "64:0:0", "64:", "64::1", "+64", " 64", "-64", "64:+0", "64:-1", "64:0:2", "64:0:3", "64:0:256",
                               "64:0:512", "64x", "", "64:0:1:", "1000000001"])
    each(FOLD, "--fold-bins", ["2", "1", "4096", "4097", "16x", "", " 16", "+16", "-16", "0"])
    each(FOLD, "--fold-rows", ["0", "-4", "512", "+5", " 5", "5x", "", "1000000000", "1000000001"])
    each(DM, "--fold", ["3.3", "3.3:-2e-3", "3.3:-2e-3:0.25", "3.3:", "1:2:3:4", "1:2:3:", "abc", "", " 3.3", "+3.3", "-3.3", "3.3x", "nan", ":1", "3.3::1", "3.3,1"])
    each(FOLD, "--fold-dm", ["20", "-1", "0", "x", "", "20x", "nan", "-0", " 20", "+20", "20:"])
    each(DM, "--ffa", ["8:13", "8", "8:", ":13", "8:13:2", "a:b", "-8:13", "8:13x", "+8:13", "8:+13", " 8:13", "8: 13", "8:-13", "", "1000000001:13", "8:1000000001", "0:0",
                       "8,13"])
    each(FFA, "--ffa-detrend", ["4", "4:9", "4:", "4:9:1", "+4:9", ":9", "4:-9", "4:9x", " 4:9", "4: 9", "", "0:0"])
    for option in ("--ffa-seg", "--ffa-dec", "--ffa-oct", "--ffa-widths"):
        each(FFA, option, ["64", "64k", "-2", "1.5", "", "+2", " 2", "0", "1000000001"])
    each(FFA, "--ffa-snr", ["7", "high", "nan", "7x", "", "-3", "inf", " 7", "+7", "7:"])
    each(CO, "--coherent-fft", ["32", "64", "128", "4096", "8192", "100", "0", "-64", "+64", " 64", "64x", "", "1000000001"])
    each(CO, "--coherent-int", ["1", "0", "-1", "+2", "2x", " 2", "", "16"])
    each(CO, "--coherent-sideband", ["+1", "-1", "1", "0", "2", "-2", "-1x", " 1", "", "-1000000001"])
    each(VO, "--voltage-units", ["1", "0", "2", "+2", " 2", "-3", "2x", "", "1000000000", "1000000001"])
    each(VO, "--voltage-history", ["8", "0", "1", "+8", " 8", "-8", "8x", ""])
    each(DM, "--inject", ["300:20:3:6", "300:20:3:6:1.5", "300:20:3:6:1.5:16", "abc", "", "300:20:3", "300:20:3:6:", "300:20:3:6:1:8:9", "300:20:3:6x", "-1:20:3:6",
                          "300.5:20:3:6", "300:-2:3:6", "300:20:-1:6", "300:20:2.5:6", "300:20:3:nan", "300:20:3:inf", "300:20:3:6:0", "300:20:3:6:-1", "300:20:3:6:1:0",
                          "300:20:3:6:1:1", "300:20:3:6:1:4096", "300:20:3:6:1:4097", "300:20:3:6:1:7.5", "300:20:3:6:1000", "300:20:3:6:512", "300:20:3:6:513", "+300:20:3:6",
                          " 300:20:3:6", "300: 20:3:6", "0:0:0:0", "9000000000000000:20:3:6", "9000000000000002:20:3:6", "300:20:1000000000:6", "300:20:1000000001:6",
                          "300:20:3:-6", "300,20,3,6"])
    each(DM, "--inject-train", ["3.3:20:3:0.5", "3.3:20:3:0.5:0.1", "3.3:20:3:0.5:0.1:32", "3.3:20:3", "3.3:-1:3:0.5", "3.3:20:3:0.5:0", "3.3:20:3:0.5:1", "3.3:20:3:0.5:1.5",
                                "3.3:20:3:0.5:0.1:1", "3.3:20:3:0.5:0.1:2", "3.3:20:3:0.5:0.1:4096", "3.3:20:3:0.5:0.1:4097", "3.3:20:3:0.5:0.1:32.5", "inf:20:3:0.5",
                                "3.3:20:2.5:0.5", "3.3:20:3:0.5:0.1:32:1", "3.3:20:3:0.5x", ""])
    c += [DM + ["--inject", "300:20:3:6", "--inject", "abc"], DM + ["--inject", "300:20:3:6", "--inject-train", "3.3:20:3:0.5", "--inject-out", "x"]]
    each(NUL, "-y", ["0", "5", "1", "4", "2:", "2:-1", "2:0", "2:4.5", "2x", "2:4x", "", "+2", " 2", "-1", "2:nan", "2:inf", "2,4", "x", "2: 4", "2:4:1"])
    # the lenient short options
    c += [["-g", "x"], ["-D", "7", "-a", "2", "-u", "-v"], OBS + ["-R", "2"], OBS + ["-R", "2", "-r", "1", "-I", "id"], ["-j", "x"], ["-j", "-1", "-i", "3"],
          DM + ["-N", "x", "-T", "x"], ["-c", "3", "-k", "baab"], ["-p", T + "missing", "-d", T + "missing", "-s", T + "missing", "-o", "out.py"], ["-w", "w", "-K", "ring"],
          OBS + DM + ["-W", "w", "-Q", "q", "-X"], ["positional"], ["--", "-S", "8"], ["-S8"], ["--fold=3.3"], DM + ["--fold=3.3"],
          OBS + SPS + ["-N", "4", "-T", "0.02", "-C", "c", "--events", "e", "--stamps", "s", "--voltages", "v", "-n", "3", "-z", "--inject", "300:20:3:6", "--inject-out", "t",
                       "--fold", "3.3", "--ffa", "8:13"]]
    return c


def run_one(beam, tmp, index, argv):
    """One command line in a directory of its own: exit status, both streams and whatever files it left, the temporary directory and the
    program's own path written as {tmp} and {beam}."""
    cwd = os.path.join(tmp, "run%04d" % index)
    os.makedirs(cwd)
    r = subprocess.run([beam] + [a.replace("{tmp}", tmp) for a in argv], cwd=cwd, capture_output=True, timeout=120)

    def text(b):
        return b.decode("utf-8", "backslashreplace").replace(tmp, "{tmp}").replace(beam, "{beam}")

    files = {}
    for name in sorted(os.listdir(cwd)):
        with open(os.path.join(cwd, name), "rb") as fp:
            files[name] = text(fp.read())
    return {"argv": argv, "rc": r.returncode, "stdout": text(r.stdout), "stderr": text(r.stderr), "files": files}


def run_all(beam, tmp, argvs):
    make_inputs(tmp)
    with ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(lambda ia: run_one(beam, tmp, ia[0], ia[1]), enumerate(argvs)))


def _reaches_the_device(rec):
    return rec["rc"] != 0 and rec["stderr"].startswith("GPUassert:") and "beam:" not in rec["stderr"]


def test_the_driver_answers_every_recorded_command_line_as_recorded(tmp_path):
    import torch

    from dsabeamformer_amd import build as b

    b.build()
    with open(FIXTURE) as fp:
        want = json.load(fp)
    assert [r["argv"] for r in want] == corpus()   # the fixture is the record of THIS list
    assert len(want) >= 300 and sum(1 for r in want if not r.get("device")) >= 200
    if torch.cuda.is_available():   # with a device these would start a run
        want = [r for r in want if not r.get("device")]
    got = run_all(b.BEAM, str(tmp_path), [r["argv"] for r in want])
    wrong = []
    for w, g in zip(want, got):
        if w.get("device"):
            if not _reaches_the_device(g) or g["stdout"] or g["files"]:
                wrong.append((w["argv"], "should pass every check and fail at the device", g))
        elif {k: w[k] for k in ("rc", "stdout", "stderr", "files")} != {k: g[k] for k in ("rc", "stdout", "stderr", "files")}:
            wrong.append((w, g))
    assert not wrong, "%d of %d command lines differ from the record, the first: %r" % (len(wrong), len(want), wrong[0])


if __name__ == "__main__":
    import tempfile

    with tempfile.TemporaryDirectory() as scratch:
        records = run_all(os.path.abspath(sys.argv[1]), os.path.realpath(scratch), corpus())
    for n, rec in enumerate(records):
        if _reaches_the_device(rec):
            assert not rec["stdout"] and not rec["files"], rec
            records[n] = {"argv": rec["argv"], "device": True}
    with open(FIXTURE, "w") as fp:
        json.dump(records, fp, indent=0, sort_keys=True)
        fp.write("\n")
    print("%d command lines, %d of them reach the device" % (len(records), sum(1 for r in records if r.get("device"))))
