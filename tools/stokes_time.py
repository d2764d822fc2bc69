#!/usr/bin/env python3
"""Times of the full-Stokes follow-up beams (docs/STOKES.md) over the production block launch's input -- 128 gemm-units of the C3
geometry resident on the device (1 GiB), and the same 128 units of the DEBUG geometry (n_avg 1, 64 MiB) -- HIP events around every
launch, the measurements taken in turn, round after round, in one process on one box:

  (a)   bf_stokes_device, 16 beams, n_int = n_avg
  (a')  bf_stokes_device, 4 beams, n_int = 1 (writes four times the input's bytes)
  (b)   a device-to-device hipMemcpyAsync of the same input bytes
  (c)   bf_sk_device: the same bytes read once with a few operations per sample
  (d)   bf_beamform_device over the same input alone
  (e)   bf_beamform_device with a bf_stokes_push (16 beams, n_int = n_avg) of the same units behind it on the same queue

  python tools/stokes_time.py [--rounds R] [--reps N] [--units U]

The bar of docs/STOKES.md: (a) <= (d) at C3, medians of the same run; the rest is reported."""
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
    # a block holds the units of one launch, so that one push takes them; a second, small handle carries the (a') stage, whose result
    # sets (never used here: bf_stokes_device writes the caller's output) are sized by ITS block
    shape = dict(n_out_per_gemm=16, n_gemms_per_block=a.units, n_blocks_on_gpu=1)
    small = dict(n_out_per_gemm=16, n_gemms_per_block=8, n_blocks_on_gpu=1)
    for label, make in (("c3", bfm.production_config), ("debug", bfm.debug_config)):
        cfg = make(**shape)
        bf, bf_small = bfm.Beamformer(cfg), bfm.Beamformer(make(**small))
        w = host.make_weights(host.default_positions(cfg.n_ant), host.default_directions(cfg.n_beams), cfg.n_freq, chan0=0, gpu=0)
        bf.set_weights(w)
        wide = api.StokesBeams(bf, None, max_in_flight=1)                 # 16 beams, n_int = n_avg
        wide.set_weights(w, list(range(0, 256, 16)))
        fine = api.StokesBeams(bf_small, 1, max_in_flight=1)              # 4 beams, every sample
        fine.set_weights(w, [0, 100, 200, 255])
        nbytes = bf.bytes_per_gemm * a.units
        d_in = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
        d_copy = torch.empty_like(d_in)
        n_rows = a.units * cfg.n_out_per_gemm * cfg.n_freq
        d_wide = torch.zeros(a.units * wide.entries * 4, dtype=torch.int64, device="cuda")
        d_fine = torch.zeros(a.units * fine.entries * 4, dtype=torch.int64, device="cuda")
        d_mom = torch.zeros(bf.sk_entries * 2, dtype=torch.int64, device="cuda")
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
                if wide.pending:
                    wide.collect()                                        # (the set's copy runs on the stage's own queue: not timed)
            return out

        def beamform_and_push():
            bf.beamform(d_in, a.units, d_det, stream.cuda_stream)
            wide.push(d_in, a.units, stream.cuda_stream)

        runs = {
            "a_stokes_16_beams_n_avg": lambda: wide.compute(d_in, a.units, d_wide, stream.cuda_stream),
            "a1_stokes_4_beams_n_int_1": lambda: fine.compute(d_in, a.units, d_fine, stream.cuda_stream),
            "b_copy_of_the_input": lambda: hip.hipMemcpyAsync(C.c_void_p(d_copy.data_ptr()), C.c_void_p(d_in.data_ptr()), C.c_size_t(nbytes), 3,
                                                              C.c_void_p(stream.cuda_stream)),
            "c_voltage_moments": lambda: bf.voltage_moments(d_in, a.units, d_mom, False, stream.cuda_stream),
            "d_beamform_alone": lambda: bf.beamform(d_in, a.units, d_det, stream.cuda_stream),
            "e_beamform_and_push": beamform_and_push,
        }
        t = {k: [] for k in runs}
        for fn in runs.values():                       # warm-up: every kernel and copy
            timed(fn, 3)
        for _ in range(a.rounds):
            for k, fn in runs.items():
                t[k] += timed(fn, a.reps)
        print("%s: %d gemm-units, %.0f MiB of input, %d antennas; %d rounds x %d launches; output (a) %.0f MiB, (a') %.0f MiB"
              % (label, a.units, nbytes / 2 ** 20, cfg.n_ant, a.rounds, a.reps, d_wide.numel() / 2 ** 17, d_fine.numel() / 2 ** 17))
        r = {}
        for k, v in t.items():
            v = sorted(v)
            r[k] = {"median_us": 1e3 * v[len(v) // 2], "min_us": 1e3 * v[0], "max_us": 1e3 * v[-1], "n": len(v)}
            print("  %-28s median %9.1f us   min %9.1f   max %9.1f   (%d)   %6.2f TB/s of input at the median"
                  % (k, r[k]["median_us"], r[k]["min_us"], r[k]["max_us"], len(v), nbytes / r[k]["median_us"] / 1e6))
        am, dm = r["a_stokes_16_beams_n_avg"]["median_us"], r["d_beamform_alone"]["median_us"]
        r["bar_a_le_d"] = bool(am <= dm)
        print("  (a) <= (d): %.1f <= %.1f  %s" % (am, dm, "met" if r["bar_a_le_d"] else "MISSED"))
        res[label] = r
        wide.close()
        fine.close()
        bf.close()
        bf_small.close()
        del d_in, d_copy, d_wide, d_fine, d_mom, d_det
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
