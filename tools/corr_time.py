#!/usr/bin/env python3
"""Times of the correlator (docs/CORRELATOR.md) over the production block launch's input -- 128 gemm-units of the C3 geometry resident
on the device (1 GiB), and the same 128 units of the DEBUG geometry (n_avg 1, 64 MiB) -- HIP events around every launch, a warm-up,
the measurements taken in turn over three rounds of eight launches, in one process on one box:

  (a)  bf_correlate_device (store, not accumulate)
  (b)  a device-to-device hipMemcpyAsync of the same input bytes
  (c)  bf_beamform_device over the same bytes with calibrated weights (bench.calibrated_weights: the general kernel)

  python tools/corr_time.py [--rounds R] [--reps N] [--units U]

The bar of docs/CORRELATOR.md: (a) <= (c) at C3 -- the beamformer the correlator sits beside is the yardstick; (a) / (b) is reported."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--units", type=int, default=128)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    import bench
    import dsabeamformer_amd as bfm
    from dsabeamformer_amd import _lib, host

    hip = _lib._preload_hip_runtime()
    stream = torch.cuda.Stream()
    res = {"device": torch.cuda.get_device_name(0), "units": a.units}
    for label, cfg in (("c3", bfm.production_config(n_out_per_gemm=16)), ("debug", bfm.debug_config(n_out_per_gemm=16))):
        bf = bfm.Beamformer(cfg)
        w = host.make_weights(host.default_positions(cfg.n_ant), host.default_directions(cfg.n_beams), cfg.n_freq, chan0=0, gpu=0)
        bf.set_weights(bench.calibrated_weights(w))
        kernel = bf.kernel_info(a.units)["kernel"]
        assert "PAIRED" not in kernel and "FOLD" not in kernel, kernel          # calibrated weights: the general kernel
        nbytes = bf.bytes_per_gemm * a.units
        d_in = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
        d_copy = torch.empty_like(d_in)
        d_vis = torch.zeros(bf.corr_entries * 2, dtype=torch.int64, device="cuda")
        d_det = torch.zeros(a.units * cfg.n_out_per_gemm * cfg.n_freq * cfg.n_beams, dtype=torch.float32, device="cuda")

        def timed(fn, n):
            out = []
            for _ in range(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                stream.synchronize()
                out.append(e0.elapsed_time(e1))
            return out

        runs = {
            "a_correlate": lambda: bf.correlate(d_in, a.units, d_vis, False, stream.cuda_stream),
            "b_copy_of_the_input": lambda: hip.hipMemcpyAsync(C.c_void_p(d_copy.data_ptr()), C.c_void_p(d_in.data_ptr()), C.c_size_t(nbytes), 3,
                                                              C.c_void_p(stream.cuda_stream)),
            "c_beamform_general": lambda: bf.beamform(d_in, a.units, d_det, stream.cuda_stream),
        }
        t = {k: [] for k in runs}
        for fn in runs.values():                       # warm-up: every kernel and the copy
            timed(fn, 3)
        for _ in range(a.rounds):
            for k, fn in runs.items():
                t[k] += timed(fn, a.reps)
        cols = a.units * cfg.n_out_per_gemm * cfg.n_avg
        print("%s: %d gemm-units, %.0f MiB of input, %d columns per polarisation, %d int64 of output; %d rounds x %d launches; beamformer: %s"
              % (label, a.units, nbytes / 2 ** 20, cols, d_vis.numel(), a.rounds, a.reps, kernel))
        r = {}
        for k, v in t.items():
            v = sorted(v)
            r[k] = {"median_us": 1e3 * v[len(v) // 2], "min_us": 1e3 * v[0], "max_us": 1e3 * v[-1], "n": len(v)}
            print("  %-22s median %9.1f us   min %9.1f   max %9.1f   (%d)   %6.2f TB/s of input at the median"
                  % (k, r[k]["median_us"], r[k]["min_us"], r[k]["max_us"], len(v), nbytes / r[k]["median_us"] / 1e6))
        am, bm, cm = (r[k]["median_us"] for k in runs)
        r["a_over_b"] = am / bm
        r["bar_a_le_c"] = bool(am <= cm)
        print("  (a) / (b) = %.2f;   bar (a) <= (c): %.1f <= %.1f  %s" % (am / bm, am, cm, "met" if r["bar_a_le_c"] else "MISSED"))
        res[label] = r
        bf.close()
        del d_in, d_copy, d_vis, d_det
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
