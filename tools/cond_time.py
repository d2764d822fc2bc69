#!/usr/bin/env python3
"""Times of the conditioning stage (docs/CONDITIONING.md), HIP events around every call, the four measurements taken in turn, round
after round, in one process on one box:

  (a)  bf_cond_push on resident rows (window 8, zero-DM on, automatic mask at 5)
  (b)  a device-to-device hipMemcpyAsync of the same rows
  (c)  bf_dm_stream_push with the stage attached
  (c0) bf_dm_stream_push without it

  python tools/cond_time.py [--shape c3|band] [--rounds R] [--pushes N]

c3: the production push of BASELINE's C3, 512 rows x 256 channels x 256 beams (128 MiB); band: a gathered band of 2048 channels
(1 GiB per push, 8 DM trials).  The bar of docs/CONDITIONING.md: (a) <= 2 x (b).  The DM pushes take the zero-copy feed
(bf_dm_stream_reserve); their rows are written before the first event is recorded.  One GPU process; run it under `timeout`."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SHAPES = {"c3": dict(n_freq=256, n_dm=64), "band": dict(n_freq=2048, n_dm=8)}
N_T, N_BEAMS = 512, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="c3")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pushes", type=int, default=8)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import dsabeamformer_amd as bfm
    from dsabeamformer_amd import _lib, api, host

    n_freq, n_dm = SHAPES[a.shape]["n_freq"], SHAPES[a.shape]["n_dm"]
    bf = bfm.Beamformer(bfm.production_config())
    hip = _lib._preload_hip_runtime()
    freq = np.linspace(1.53, 1.28, n_freq).astype(np.float32)
    ladder = host.dm_trials(dm_max=250.0)
    dms = ladder[:: max(1, len(ladder) // n_dm)][:n_dm]
    delays = host.dm_delays(dms, freq, float(freq[0]), 0.131)
    stream = torch.cuda.Stream()
    n = N_T * n_freq * N_BEAMS
    rows = torch.rand(n, device="cuda") * 1e3 + 10.0
    work = rows.clone()
    copy_dst = torch.empty_like(rows)
    kw = dict(baseline_pushes=8, zero_dm=True, auto_threshold=5.0)
    cond_alone = api.Conditioner(bf, n_freq, N_T, **kw)
    cond_attached = api.Conditioner(bf, n_freq, N_T, **kw)
    dm_plain = api.DmStream(bf, delays, n_freq, N_T)
    dm_cond = api.DmStream(bf, delays, n_freq, N_T)
    dm_cond.attach_conditioner(cond_attached)
    t = {"a_cond_push": [], "b_copy": [], "c_dm_push_with_cond": [], "c0_dm_push": []}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1), out

    def copy_rows(dst, src):
        assert hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(n * 4), 3, C.c_void_p(stream.cuda_stream)) == 0

    def cond_pushes(k):
        out = []
        for _ in range(k):
            copy_rows(work.data_ptr(), rows.data_ptr())            # raw rows again (outside the timed window)
            out.append(timed(lambda: cond_alone.push(work, N_T, stream.cuda_stream))[0])
        return out

    def copies(k):
        return [timed(lambda: copy_rows(copy_dst.data_ptr(), rows.data_ptr()))[0] for _ in range(k)]

    def dm_pushes(dm, k):
        out = []
        for _ in range(k):
            dst = dm.reserve(N_T, stream.cuda_stream)
            copy_rows(dst, rows.data_ptr())
            ms, (_, n_out) = timed(lambda: dm.push(dst, N_T, None, stream.cuda_stream))
            if n_out == N_T:            # (the first pushes fill the delay window: shorter chunks)
                out.append(ms)
        return out

    # warm-up: every kernel and copy once, the delay windows and the statistics' window filled
    cond_pushes(9), copies(4), dm_pushes(dm_cond, 9), dm_pushes(dm_plain, 4)
    for _ in range(a.rounds):
        t["a_cond_push"] += cond_pushes(a.pushes)
        t["b_copy"] += copies(a.pushes)
        t["c_dm_push_with_cond"] += dm_pushes(dm_cond, a.pushes)
        t["c0_dm_push"] += dm_pushes(dm_plain, a.pushes)
    print("device: %s; shape %s; %d rounds x %d pushes; push = %d rows x %d channels x %d beams (%.0f MiB), %d DM trials, largest delay %d"
          % (torch.cuda.get_device_name(0), a.shape, a.rounds, a.pushes, N_T, n_freq, N_BEAMS, n * 4 / 2 ** 20, n_dm, int(delays.max())))
    res = {"shape": a.shape}
    for name, v in t.items():
        v = sorted(v)
        res[name] = {"median_us": 1e3 * v[len(v) // 2], "min_us": 1e3 * v[0], "max_us": 1e3 * v[-1], "n": len(v)}
        print("  %-22s median %9.1f us   min %9.1f   max %9.1f   (%d calls)" % (name, res[name]["median_us"], res[name]["min_us"], res[name]["max_us"], len(v)))
    av, bv = res["a_cond_push"]["median_us"], res["b_copy"]["median_us"]
    res["c_minus_c0_us"] = res["c_dm_push_with_cond"]["median_us"] - res["c0_dm_push"]["median_us"]
    res["bar_a_le_2b"] = bool(av <= 2 * bv)
    print("  (c) - (c0): %.1f us" % res["c_minus_c0_us"])
    print("  bar (a) <= 2 x (b): %.1f <= %.1f  %s" % (av, 2 * bv, "met" if res["bar_a_le_2b"] else "MISSED"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
