#!/usr/bin/env python3
"""Times of the periodicity search beside the DM push (docs/PERIODICITY.md section 8): 64 trials x 256 beams, pushes of 512 times,
tdec 4, n_seg 8192, base periods 64 .. 127, 3 octaves, 5 widths; HIP events, one process, a warm-up, then rounds with the arms taken
in turn:

  (a)  a DM push on the parent commit's library    [--parent-lib LIB, through DSABF_LIB_PATH, in a subprocess per round]
  (a0) a DM push with this build, nothing attached -- in a subprocess per round exactly as (a), so the two differ in the library
       and in nothing else
  (b)  the search of one full segment alone: the push of the segment's last 4 times (one decimation group, then the search)
  (b') the same on the parent commit's library     [--parent-lib LIB, in a subprocess per round, as (a)]
  (f)  (b) on a second stage with the detrend on   [--detrend BLK:WIN: the detrend kernel between the decimation and the search]
  (c)  a push of 512 times that only accumulates
  (d)  a device-to-device copy of one segment's series, n_dm x n_beams x n_seg floats
  (e)  a device-to-pinned copy of one segment's records

  python tools/ffa_time.py [--rounds R] [--pushes N] [--parent-lib variants/parent/libdsabf.so] [--detrend 64:33]

Bar 1: median (a0) <= median (a) + (max (a) - min (a)); with --detrend also median (b) <= median (b') + (max (b') - min (b')): the
detrend off costs nothing.  Bar 2: max (b) -- max (f) with --detrend -- + the (c) pushes of one segment (at max (c)) below the
segment's sky time, n_seg x tdec rows x 131 us.  (b) / (n_oct x (d)), (e), and ((f) - (b)) against (d) and (b) are reported."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
N_DM, N_T, N_BEAMS, N_FREQ = 64, 512, 256, 256
TDEC, N_SEG, N_OCT, P_LO, P_HI, K = 4, 8192, 3, 64, 128, 5
ROW_US = 131.0


def setup():
    sys.path.insert(0, ROOT)
    import torch

    import dsabeamformer_amd as bfm
    from dsabeamformer_amd import _lib, api, host

    bf = bfm.Beamformer(bfm.production_config())
    freq = [host.channel_frequency(0, c) for c in range(N_FREQ)]
    ladder = host.dm_trials(dm_max=250.0)
    dms = ladder[:: max(1, len(ladder) // N_DM)][:N_DM]
    delays = host.dm_delays(dms, freq, freq[0], 0.131)
    assert delays.shape == (N_DM, N_FREQ)
    return torch, bfm, _lib, api, bf, delays


def time_dm_pushes(torch, hip, dm, rows, n, stream):
    """n pushes of N_T rows (zero-copy feed; the rows are written before the first event is recorded): the event times in ms."""
    out = []
    for _ in range(n):
        dst = dm.reserve(N_T, stream.cuda_stream)
        assert hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(rows.data_ptr()), C.c_size_t(rows.numel() * 4), 3, C.c_void_p(stream.cuda_stream)) == 0
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        _, n_out = dm.push(dst, N_T, None, stream.cuda_stream)
        b.record(stream)
        stream.synchronize()
        if n_out == N_T:
            out.append(a.elapsed_time(b))
    return out


def timed(torch, stream, call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    call()
    b.record(stream)
    stream.synchronize()
    return a.elapsed_time(b)


def child_dm_only(a):
    """(a) / (a0) on the library DSABF_LIB_PATH names (or the product): prints the times of one round as JSON."""
    torch, bfm, _lib, api, bf, delays = setup()
    hip = _lib._preload_hip_runtime()
    stream = torch.cuda.Stream()
    rows = torch.rand(N_T * N_FREQ * N_BEAMS, device="cuda")
    dm = api.DmStream(bf, delays, N_FREQ, N_T)
    time_dm_pushes(torch, hip, dm, rows, a.warm, stream)
    print(json.dumps(time_dm_pushes(torch, hip, dm, rows, a.pushes, stream)))


class Segments:
    """One stage fed the same chunk again and again, a whole segment at a time."""

    def __init__(self, torch, api, bf, stream, chunk, detrend=None):
        kw = {"detrend": detrend} if detrend else {}          # (the parent commit's api has no such argument)
        self.ffa = api.PeriodicitySearch(bf, N_DM, TDEC, N_SEG, N_OCT, P_LO, P_HI, K, N_T, max_in_flight=1, threshold=8.0, **kw)
        self.torch, self.stream, self.chunk, self.first_t = torch, stream, chunk, 0

    def push(self, n_t):
        self.ffa.push(self.chunk, n_t, self.first_t, self.stream.cuda_stream)
        self.first_t += n_t

    def one(self, accumulating):
        """A whole segment: pushes of 512 that accumulate (their times appended to `accumulating`, a list or None), 508 more times,
        then the 4 that complete it.  Returns (ms of the completing push, seconds of bf_ffa_collect on the host)."""
        for i in range(N_SEG * TDEC // N_T - 1):
            ms = timed(self.torch, self.stream, lambda: self.push(N_T))
            if accumulating is not None and i == 0:
                accumulating.append(ms)
        self.push(N_T - TDEC)
        self.stream.synchronize()
        ms = timed(self.torch, self.stream, lambda: self.push(TDEC))
        w0 = time.perf_counter()
        self.ffa.collect()
        return ms, time.perf_counter() - w0


def child_search(a):
    """(b') on the library DSABF_LIB_PATH names: a warm-up segment, then the times of `pushes` segments as JSON."""
    torch, bfm, _lib, api, bf, delays = setup()
    stream = torch.cuda.Stream()
    seg = Segments(torch, api, bf, stream, torch.randn(N_DM * N_T * N_BEAMS, device="cuda"))
    seg.one(None)
    print(json.dumps([seg.one(None)[0] for _ in range(a.pushes)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pushes", type=int, default=8)
    ap.add_argument("--warm", type=int, default=6)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--detrend", default=None, help="BLK:WIN: arm (f), and (b') if --parent-lib is given")
    ap.add_argument("--child-dm-only", action="store_true")
    ap.add_argument("--child-search", action="store_true")
    a = ap.parse_args()
    if a.child_dm_only:
        return child_dm_only(a)
    if a.child_search:
        return child_search(a)
    detrend = tuple(int(v) for v in a.detrend.split(":")) if a.detrend else None
    torch, bfm, _lib, api, bf, delays = setup()
    hip = _lib._preload_hip_runtime()
    stream = torch.cuda.Stream()
    chunk = torch.randn(N_DM * N_T * N_BEAMS, device="cuda")                  # one chunk [n_dm][512][n_beams], pushed again and again
    series = torch.empty(N_DM * N_BEAMS * N_SEG, device="cuda")
    series_copy = torch.empty_like(series)
    plain = Segments(torch, api, bf, stream, chunk)
    detrended = Segments(torch, api, bf, stream, chunk, detrend) if detrend else None
    n_rec_bytes = N_OCT * (P_HI - P_LO) * K * N_DM * N_BEAMS * 8
    rec_dev = torch.empty(n_rec_bytes // 4, device="cuda")
    rec_host = torch.empty(n_rec_bytes // 4).pin_memory()
    pushes_per_segment = N_SEG * TDEC // N_T
    t = {"a_dm_push_parent_lib": [], "a0_dm_push_nothing_attached": [], "b_search_one_segment": [], "c_push_accumulates": [], "d_copy_series_d2d": [],
         "e_records_to_pinned": [], "collect_host_s": [], "b_parent_lib_search_one_segment": [], "f_search_one_segment_detrended": []}

    def d2d():
        assert hip.hipMemcpyAsync(C.c_void_p(series_copy.data_ptr()), C.c_void_p(series.data_ptr()), C.c_size_t(series.numel() * 4), 3,
                                  C.c_void_p(stream.cuda_stream)) == 0

    def d2h():
        assert hip.hipMemcpyAsync(C.c_void_p(rec_host.data_ptr()), C.c_void_p(rec_dev.data_ptr()), C.c_size_t(n_rec_bytes), 2,
                                  C.c_void_p(stream.cuda_stream)) == 0

    plain.one(None)                                                            # warm-up: every kernel once
    if detrended:
        detrended.one(None)
    timed(torch, stream, d2d)
    timed(torch, stream, d2h)
    parent_env = dict(os.environ, DSABF_LIB_PATH=os.path.abspath(a.parent_lib)) if a.parent_lib else None
    for r in range(a.rounds):
        for name, env, mode in (("a_dm_push_parent_lib", parent_env, "--child-dm-only"),
                                ("a0_dm_push_nothing_attached", {k: v for k, v in os.environ.items() if k != "DSABF_LIB_PATH"}, "--child-dm-only"),
                                ("b_parent_lib_search_one_segment", parent_env if detrend else None, "--child-search")):
            if env is None:
                continue
            p = subprocess.run([sys.executable, os.path.abspath(__file__), mode, "--pushes", str(a.pushes), "--warm", str(a.warm)],
                               env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:   # an abort, a fault or a time limit in the child: nothing more is started on this GPU
                print("%s: the child ended with status %d; stopping: %s" % (name, p.returncode, (p.stdout + p.stderr)[-600:]))
                sys.exit(1)
            t[name] += json.loads(p.stdout.strip().splitlines()[-1])
        for i in range(a.pushes):
            ms, host_s = plain.one(t["c_push_accumulates"])
            t["b_search_one_segment"].append(ms)
            t["collect_host_s"].append(host_s * 1e3)
            if detrended:
                t["f_search_one_segment_detrended"].append(detrended.one(None)[0])
            t["d_copy_series_d2d"].append(timed(torch, stream, d2d))
            t["e_records_to_pinned"].append(timed(torch, stream, d2h))
    print("device: %s; %d rounds x %d; %d trials x %d beams, pushes of %d, tdec %d, n_seg %d, p %d .. %d, %d octaves, %d widths; series %.0f MiB, records %.0f MiB"
          % (torch.cuda.get_device_name(0), a.rounds, a.pushes, N_DM, N_BEAMS, N_T, TDEC, N_SEG, P_LO, P_HI - 1, N_OCT, K, series.numel() * 4 / 2 ** 20,
             n_rec_bytes / 2 ** 20))
    res = {}
    for name, v in t.items():
        if not v:
            continue
        v = sorted(v)
        res[name] = {"median_us": 1e3 * v[len(v) // 2], "min_us": 1e3 * v[0], "max_us": 1e3 * v[-1], "n": len(v)}
        print("  %-32s median %11.1f us   min %11.1f   max %11.1f   (n %d)" % (name, res[name]["median_us"], res[name]["min_us"], res[name]["max_us"], len(v)))
    sky_us = N_SEG * TDEC * ROW_US
    search = res["f_search_one_segment_detrended" if detrend else "b_search_one_segment"]
    busy_us = search["max_us"] + pushes_per_segment * res["c_push_accumulates"]["max_us"]
    res["bar2_segment_below_sky_time"] = bool(busy_us < sky_us)
    res["bar2_ratio"] = busy_us / sky_us
    print("  bar 2, max (%s) + %d x max (c) = %.0f us below the segment's sky time (%.0f us): %s, ratio %.4f" %
          ("f" if detrend else "b", pushes_per_segment, busy_us, sky_us, "met" if res["bar2_segment_below_sky_time"] else "MISSED", res["bar2_ratio"]))
    res["b_over_octaves_d"] = res["b_search_one_segment"]["median_us"] / (N_OCT * res["d_copy_series_d2d"]["median_us"])
    print("  (b) / (n_oct x (d)) = %.1f" % res["b_over_octaves_d"])
    if "a_dm_push_parent_lib" in res:
        a0, pa = res["a0_dm_push_nothing_attached"], res["a_dm_push_parent_lib"]
        res["bar1_a0_le_a_plus_scatter"] = bool(a0["median_us"] <= pa["median_us"] + (pa["max_us"] - pa["min_us"]))
        print("  bar 1, median (a0) <= median (a) + (max (a) - min (a)): %s" % ("met" if res["bar1_a0_le_a_plus_scatter"] else "MISSED"))
    if detrend:
        b, f, d = res["b_search_one_segment"], res["f_search_one_segment_detrended"], res["d_copy_series_d2d"]
        res["detrend"] = list(detrend)
        res["f_minus_b_us"] = f["median_us"] - b["median_us"]
        res["f_minus_b_over_d"] = res["f_minus_b_us"] / d["median_us"]
        res["f_minus_b_over_b"] = res["f_minus_b_us"] / b["median_us"]
        print("  detrend %d:%d: (f) - (b) = %.1f us = %.2f x (d) = %.4f x (b)" % (detrend + (res["f_minus_b_us"], res["f_minus_b_over_d"], res["f_minus_b_over_b"])))
        if "b_parent_lib_search_one_segment" in res:
            pb = res["b_parent_lib_search_one_segment"]
            res["bar1_b_le_parent_b_plus_scatter"] = bool(b["median_us"] <= pb["median_us"] + (pb["max_us"] - pb["min_us"]))
            print("  bar 1 (detrend off), median (b) <= median (b') + (max (b') - min (b')): %s" % ("met" if res["bar1_b_le_parent_b_plus_scatter"] else "MISSED"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
