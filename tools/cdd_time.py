#!/usr/bin/env python3
"""Times of coherent dedispersion (docs/COHERENT_DEDISPERSION.md) with the protocol of tools/stokes_time.py: HIP events around every
launch, a warm-up, rounds of launches with the arms taken in turn, one process on one box.

Workload: 256 channels x 4 beams x 2 polarisations x 32768 samples of complex float32 (the beam voltages of 128 gemm-units of the C3
geometry, 512 MiB), Stokes parameters at n_int = 1, at two settings: N = 1024 with edge 30 and N = 4096 with edge 177.

  (a)   bf_cdd_stokes_device
  (a')  bf_cdd_voltages_device (reported)
  (b)   the same arithmetic as separate torch operations on the same tensor: segment gather (from a series padded beforehand, outside
        the timing), torch.fft.fft, multiply, torch.fft.ifft, slice, Stokes
  (c)   a device-to-device copy of the input

and, over 128 gemm-units of C3 packed voltages (1 GiB), reported beside the arms of docs/STOKES.md section 6:
  (v)   bf_stokes_voltages_device, 4 beams           (s1) bf_stokes_device, 4 beams, n_int = 1
  (s16) bf_stokes_device, 16 beams, n_int = n_avg

  python tools/cdd_time.py [--rounds R] [--reps N]

The bar: median (a) <= median (b) at both N, in the same run; (a) / (c) is reported."""
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
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import dsabeamformer_amd as bfm
    from dsabeamformer_amd import _lib, api, host

    hip = _lib._preload_hip_runtime()
    stream = torch.cuda.Stream()
    res = {"device": torch.cuda.get_device_name(0)}

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

    def measure(label, runs, nbytes):
        t = {k: [] for k in runs}
        for fn in runs.values():
            timed(fn, 3)
        for _ in range(a.rounds):
            for k, fn in runs.items():
                t[k] += timed(fn, a.reps)
        r = {}
        print("%s: %d rounds x %d launches, %.0f MiB of input" % (label, a.rounds, a.reps, nbytes / 2 ** 20))
        for k, v in t.items():
            v = sorted(v)
            r[k] = {"median_us": 1e3 * v[len(v) // 2], "min_us": 1e3 * v[0], "max_us": 1e3 * v[-1], "n": len(v)}
            print("  %-28s median %9.1f us   min %9.1f   max %9.1f   (%d)   %6.2f TB/s of input at the median"
                  % (k, r[k]["median_us"], r[k]["min_us"], r[k]["max_us"], len(v), nbytes / r[k]["median_us"] / 1e6))
        return r

    n_chan, K, n_time = 256, 4, 32768
    bf = bfm.Beamformer(bfm.debug_config())
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randint(-2 ** 19, 2 ** 19, (n_chan, K, 2, n_time, 2), generator=gen, device="cuda").to(torch.float32)
    xc = torch.view_as_complex(x)
    nbytes = x.numel() * 4
    d_copy = torch.empty_like(x)
    d_stokes = torch.zeros((n_time, n_chan, K, 4), dtype=torch.float32, device="cuda")
    d_volts = torch.empty_like(x)
    freq = [host.channel_frequency(0, ch) for ch in range(n_chan)]
    for n_fft, n_edge, dm in ((1024, 30, 500.0), (4096, 177, 3000.0)):
        table = api.cdd_chirp(dm, freq, 250.0 / 2048, 1, n_fft)
        stage = api.CoherentDedisperser(bf, n_chan, n_fft, n_edge, table)
        v = n_fft - 2 * n_edge
        n_seg = (n_time + v - 1) // v
        runs = {
            "a_cdd_stokes_n_int_1": lambda: stage.stokes(x, K, n_time, 1, d_stokes, stream.cuda_stream),
            "a1_cdd_voltages": lambda: stage.voltages(x, K, n_time, d_volts, stream.cuda_stream),
        }
        torch_ok = True
        try:
            padded = torch.zeros((n_chan, K, 2, n_edge + n_seg * v + n_fft), dtype=torch.complex64, device="cuda")
            padded[..., n_edge:n_edge + n_time] = xc
            idx = (torch.arange(n_seg, device="cuda") * v)[:, None] + torch.arange(n_fft, device="cuda")[None, :]
            d_table = (torch.from_numpy(table).cuda() * n_fft)[:, None, None, None, :]     # (torch's ifft carries the 1 / N itself)

            def torch_arm():
                with torch.cuda.stream(stream):
                    seg = padded[..., idx]
                    y = torch.fft.ifft(torch.fft.fft(seg, dim=-1) * d_table, dim=-1)
                    y = y[..., n_edge:n_fft - n_edge].reshape(n_chan, K, 2, -1)[..., :n_time]
                    xr, xi, yr, yi = y[:, :, 0].real, y[:, :, 0].imag, y[:, :, 1].real, y[:, :, 1].imag
                    px, py = xr * xr + xi * xi, yr * yr + yi * yi
                    out = torch.stack([px + py, px - py, 2 * (xr * yr + xi * yi), 2 * (xi * yr - xr * yi)], dim=-1)
                    return out.permute(2, 0, 1, 3).contiguous()

            ref = torch_arm()
            stage.stokes(x, K, n_time, 1, d_stokes, stream.cuda_stream)
            stream.synchronize()
            scale = float(ref[..., 0].max())
            res["n%d_largest_difference_from_torch_over_largest_I" % n_fft] = float((ref - d_stokes).abs().max()) / scale
            del ref
            runs["b_torch_separate_operations"] = torch_arm
        except Exception as e:   # no FFT library behind torch on this box: (a) / (c) alone
            torch_ok = False
            res["n%d_torch_fft" % n_fft] = "not available: %s" % str(e).splitlines()[0]
            print("torch.fft does not run here:", str(e).splitlines()[0])
        runs["c_copy_of_the_input"] = lambda: hip.hipMemcpyAsync(C.c_void_p(d_copy.data_ptr()), C.c_void_p(x.data_ptr()), C.c_size_t(nbytes), 3,
                                                                 C.c_void_p(stream.cuda_stream))
        r = measure("N = %d, edge %d (%d segments of %d valid samples)" % (n_fft, n_edge, n_seg, v), runs, nbytes)
        am, cm = r["a_cdd_stokes_n_int_1"]["median_us"], r["c_copy_of_the_input"]["median_us"]
        r["a_over_c"] = am / cm
        print("  (a) / (c) = %.2f" % r["a_over_c"])
        if torch_ok:
            bm = r["b_torch_separate_operations"]["median_us"]
            r["bar_a_le_b"] = bool(am <= bm)
            print("  (a) <= (b): %.1f <= %.1f  %s" % (am, bm, "met" if r["bar_a_le_b"] else "MISSED"))
            del padded, idx, d_table
        res["n%d" % n_fft] = r
        stage.close()
        torch.cuda.empty_cache()
    bf.close()
    del x, xc, d_copy, d_stokes, d_volts
    torch.cuda.empty_cache()

    # the beam voltages beside the Stokes arms of tools/stokes_time.py
    units = 128
    cfg = bfm.production_config(n_out_per_gemm=16, n_gemms_per_block=units, n_blocks_on_gpu=1)
    small = bfm.Beamformer(bfm.production_config(n_out_per_gemm=16, n_gemms_per_block=8, n_blocks_on_gpu=1))
    big = bfm.Beamformer(cfg)
    w = host.make_weights(host.default_positions(cfg.n_ant), host.default_directions(cfg.n_beams), cfg.n_freq, chan0=0, gpu=0)
    fine = api.StokesBeams(small, 1, max_in_flight=1)
    fine.set_weights(w, [0, 100, 200, 255])
    wide = api.StokesBeams(big, None, max_in_flight=1)
    wide.set_weights(w, list(range(0, 256, 16)))
    nbytes = big.bytes_per_gemm * units
    d_in = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
    d_v = torch.zeros(units * small._lib.bf_stokes_voltage_entries(cfg, 4) * 2, dtype=torch.float32, device="cuda")
    d_fine = torch.zeros(units * fine.entries * 4, dtype=torch.int64, device="cuda")
    d_wide = torch.zeros(units * wide.entries * 4, dtype=torch.int64, device="cuda")
    res["stokes_stage"] = measure("C3 packed voltages, %d gemm-units" % units, {
        "v_beam_voltages_4_beams": lambda: fine.voltages(d_in, units, d_v, stream.cuda_stream),
        "s1_stokes_4_beams_n_int_1": lambda: fine.compute(d_in, units, d_fine, stream.cuda_stream),
        "s16_stokes_16_beams_n_avg": lambda: wide.compute(d_in, units, d_wide, stream.cuda_stream),
    }, nbytes)
    fine.close()
    wide.close()
    small.close()
    big.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
