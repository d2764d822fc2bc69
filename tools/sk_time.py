#!/usr/bin/env python3
"""Times of the voltage moments (docs/SPECTRAL_KURTOSIS.md) over the production block launch's input -- 128 gemm-units of the C3
geometry resident on the device (1 GiB), and the same 128 units of the DEBUG geometry (n_avg 1, 64 MiB) -- HIP events around
every launch, the measurements taken in turn, round after round, in one process on one box:

  (a)  bf_sk_device (overwrite: the memset of the output and the kernel)
  (b)  a device-to-device hipMemcpyAsync of the same input bytes
  (c)  bf_incoherent_device, compact output: the same bytes read with two operations per word
  (d)  bf_beamform_device over the same input alone, and with a bf_sk_push of the same units behind it on the same queue

  python tools/sk_time.py [--rounds R] [--reps N] [--units U]

The bar of docs/SPECTRAL_KURTOSIS.md: (a) <= (b) at C3; (c) and (d) are reported."""
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

    import dsabeamformer_amd as bfm
    from dsabeamformer_amd import _lib, api, host

    hip = _lib._preload_hip_runtime()
    stream = torch.cuda.Stream()
    res = {"device": torch.cuda.get_device_name(0), "units": a.units}
    for label, cfg in (("c3", bfm.production_config(n_out_per_gemm=16)), ("debug", bfm.debug_config(n_out_per_gemm=16))):
        bf = bfm.Beamformer(cfg)
        bf.set_weights(host.make_weights(host.default_positions(cfg.n_ant), host.default_directions(cfg.n_beams), cfg.n_freq, chan0=0, gpu=0))
        stage = api.SpectralKurtosis(bf, 2)
        nbytes = bf.bytes_per_gemm * a.units
        d_in = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
        d_copy = torch.empty_like(d_in)
        n_rows = a.units * cfg.n_out_per_gemm * cfg.n_freq
        d_mom = torch.zeros(bf.sk_entries * 2, dtype=torch.int64, device="cuda")
        d_ib = torch.zeros(n_rows, dtype=torch.float32, device="cuda")
        d_det = torch.zeros(n_rows * cfg.n_beams, dtype=torch.float32, device="cuda")

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

        def beamform_and_push():
            bf.beamform(d_in, a.units, d_det, stream.cuda_stream)
            stage.push(d_in, a.units, stream.cuda_stream)

        runs = {
            "a_moments": lambda: bf.voltage_moments(d_in, a.units, d_mom, False, stream.cuda_stream),
            "b_copy_of_the_input": lambda: hip.hipMemcpyAsync(C.c_void_p(d_copy.data_ptr()), C.c_void_p(d_in.data_ptr()), C.c_size_t(nbytes), 3,
                                                              C.c_void_p(stream.cuda_stream)),
            "c_incoherent_compact": lambda: bf.incoherent(d_in, a.units, d_ib, 1, stream.cuda_stream),
            "d_beamform_alone": lambda: bf.beamform(d_in, a.units, d_det, stream.cuda_stream),
            "d_beamform_and_push": beamform_and_push,
        }
        t = {k: [] for k in runs}
        for fn in runs.values():                       # warm-up: every kernel and copy
            timed(fn, 3)
        for _ in range(a.rounds):
            for k, fn in runs.items():
                t[k] += timed(fn, a.reps)
        stage.dump()                                   # (the pushes' integration: discarded)
        stage.collect()
        print("%s: %d gemm-units, %.0f MiB of input, %d antennas, %d cells; %d rounds x %d launches"
              % (label, a.units, nbytes / 2 ** 20, cfg.n_ant, bf.sk_entries, a.rounds, a.reps))
        r = {}
        for k, v in t.items():
            v = sorted(v)
            r[k] = {"median_us": 1e3 * v[len(v) // 2], "min_us": 1e3 * v[0], "max_us": 1e3 * v[-1], "n": len(v)}
            print("  %-26s median %9.1f us   min %9.1f   max %9.1f   (%d)   %6.2f TB/s of input at the median"
                  % (k, r[k]["median_us"], r[k]["min_us"], r[k]["max_us"], len(v), nbytes / r[k]["median_us"] / 1e6))
        am, bm = r["a_moments"]["median_us"], r["b_copy_of_the_input"]["median_us"]
        r["bar_a_le_b"] = bool(am <= bm)
        print("  (a) <= (b): %.1f <= %.1f  %s" % (am, bm, "met" if r["bar_a_le_b"] else "MISSED"))
        res[label] = r
        stage.close()
        bf.close()
        del d_in, d_copy, d_mom, d_ib, d_det
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
