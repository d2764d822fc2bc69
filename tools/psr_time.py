#!/usr/bin/env python3
"""Times of the pulsar fold beside the DM push at the production DM shape (tools/sps_time.py's stage: 64 trials, pushes of 512 rows of
256 channels x 256 beams), HIP events, one process, a warm-up, then rounds with the arms taken in turn:

  (a)  a DM push on the parent commit's library    [--parent-lib LIB, through DSABF_LIB_PATH, in a subprocess per round]
  (a0) a DM push with this build, no folder attached -- in a subprocess per round exactly as (a), so the two differ in the library
       and in nothing else
  (b)  bf_psr_push alone, 1 pulsar, 64 bins: at about 30 rows per bin, and at about 1 row per bin
  (c)  the same two at 4 pulsars
  (d)  a device-to-device copy of the same rows: the read floor (it also writes them)
  (e)  a DM push with the folder of (b), 30 rows per bin, attached

  python tools/psr_time.py [--rounds R] [--pushes N] [--parent-lib variants/parent/libdsabf.so]

The bars of docs/PULSAR_FOLDING.md: median (a0) <= median (a) + (max (a) - min (a)); every (b) below the sky time of its rows,
512 x 131 us = 67 ms.  (b) / (d) and (e) / (a0) are reported."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
N_DM, N_T, N_BEAMS, N_FREQ, N_BINS = 64, 512, 256, 256, 64
ROW_US = 131.0
ONE = 1 << 64


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


def timed(torch, stream, n, call):
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        stream.synchronize()
        out.append(a.elapsed_time(b))
    return out


def child_dm_only(a):
    """(a) / (a0) on the library DSABF_LIB_PATH names (or the product): prints the times of one round as JSON."""
    torch, bfm, _lib, api, bf, delays = setup()
    hip = _lib._preload_hip_runtime()
    stream = torch.cuda.Stream()
    rows = torch.rand(N_T * N_FREQ * N_BEAMS, device="cuda")
    dm = api.DmStream(bf, delays, N_FREQ, N_T)
    time_dm_pushes(torch, hip, dm, rows, a.warm, stream)
    print(json.dumps(time_dm_pushes(torch, hip, dm, rows, a.pushes, stream)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pushes", type=int, default=8)
    ap.add_argument("--warm", type=int, default=6)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child-dm-only", action="store_true")
    a = ap.parse_args()
    if a.child_dm_only:
        return child_dm_only(a)
    torch, bfm, _lib, api, bf, delays = setup()
    hip = _lib._preload_hip_runtime()
    stream = torch.cuda.Stream()
    rows = torch.rand(N_T * N_FREQ * N_BEAMS, device="cuda")
    copy = torch.empty_like(rows)
    n_bytes = rows.numel() * 4

    def models(n_psr, rows_per_bin):   # a few per cent apart, so that the pulsars' bins change at different rows
        return [(k * ONE // 7, int(ONE / (N_BINS * rows_per_bin) * (1.0 + 0.03 * k)), 0, 0) for k in range(n_psr)]

    folders = {}
    for n_psr in (1, 4):
        for rpb in (30, 1):
            folders["%s_fold_%dpsr_%drows_per_bin" % ("b" if n_psr == 1 else "c", n_psr, rpb)] = api.PulsarFolder(
                bf, N_FREQ, N_T, N_BINS, models(n_psr, rpb), delays[[(17 * k + 5) % N_DM for k in range(n_psr)]])
    dm_fold = api.DmStream(bf, delays, N_FREQ, N_T)
    attached = api.PulsarFolder(bf, N_FREQ, N_T, N_BINS, models(1, 30), delays[[5]])
    dm_fold.attach_folder(attached)
    t = {"a_dm_push_parent_lib": [], "a0_dm_push_no_folder": [], "d_copy_d2d": [], "e_dm_push_folder_attached": []}
    t.update({k: [] for k in folders})

    def d2d():
        assert hip.hipMemcpyAsync(C.c_void_p(copy.data_ptr()), C.c_void_p(rows.data_ptr()), C.c_size_t(n_bytes), 3, C.c_void_p(stream.cuda_stream)) == 0

    # warm-up: every kernel once, the delay window filled
    for f in folders.values():
        timed(torch, stream, 2, lambda: f.push(rows, N_T, stream.cuda_stream))
    timed(torch, stream, 2, d2d)
    time_dm_pushes(torch, hip, dm_fold, rows, a.warm, stream)
    for r in range(a.rounds):
        for name, env in (("a_dm_push_parent_lib", dict(os.environ, DSABF_LIB_PATH=os.path.abspath(a.parent_lib)) if a.parent_lib else None),
                          ("a0_dm_push_no_folder", {k: v for k, v in os.environ.items() if k != "DSABF_LIB_PATH"})):
            if env is None:
                continue
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-dm-only", "--pushes", str(a.pushes), "--warm", str(a.warm)],
                               env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:   # an abort, a fault or a time limit in the child: nothing more is started on this GPU
                print("%s: the child ended with status %d; stopping: %s" % (name, p.returncode, (p.stdout + p.stderr)[-600:]))
                sys.exit(1)
            t[name] += json.loads(p.stdout.strip().splitlines()[-1])
        for name, f in folders.items():
            t[name] += timed(torch, stream, a.pushes, lambda: f.push(rows, N_T, stream.cuda_stream))
        t["d_copy_d2d"] += timed(torch, stream, a.pushes, d2d)
        t["e_dm_push_folder_attached"] += time_dm_pushes(torch, hip, dm_fold, rows, a.pushes, stream)
    print("device: %s; %d rounds x %d; push = %d rows of %d x %d (%.0f MiB), %d bins" %
          (torch.cuda.get_device_name(0), a.rounds, a.pushes, N_T, N_FREQ, N_BEAMS, n_bytes / 2 ** 20, N_BINS))
    res = {}
    for name, v in t.items():
        if not v:
            continue
        v = sorted(v)
        res[name] = {"median_us": 1e3 * v[len(v) // 2], "min_us": 1e3 * v[0], "max_us": 1e3 * v[-1], "n": len(v)}
        print("  %-32s median %9.1f us   min %9.1f   max %9.1f   (n %d)" % (name, res[name]["median_us"], res[name]["min_us"], res[name]["max_us"], len(v)))
    sky_us = N_T * ROW_US
    res["bar2_fold_below_sky_time"] = bool(all(res[k]["max_us"] < sky_us for k in folders))
    print("  bar 2, every fold push below the sky time of its rows (%.0f us): %s" % (sky_us, "met" if res["bar2_fold_below_sky_time"] else "MISSED"))
    d = res["d_copy_d2d"]["median_us"]
    for k in folders:
        res[k + "_over_d"] = res[k]["median_us"] / d
        print("  %-32s / (d) = %.2f" % (k, res[k + "_over_d"]))
    a0 = res["a0_dm_push_no_folder"]
    res["e_over_a0"] = res["e_dm_push_folder_attached"]["median_us"] / a0["median_us"]
    print("  (e) / (a0) = %.3f" % res["e_over_a0"])
    if "a_dm_push_parent_lib" in res:
        pa = res["a_dm_push_parent_lib"]
        res["bar1_a0_le_a_plus_scatter"] = bool(a0["median_us"] <= pa["median_us"] + (pa["max_us"] - pa["min_us"]))
        print("  bar 1, median (a0) <= median (a) + (max (a) - min (a)): %s" % ("met" if res["bar1_a0_le_a_plus_scatter"] else "MISSED"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
