#!/usr/bin/env python3
"""Times of Faraday synthesis (docs/FARADAY.md) with the protocol of tools/cdd_time.py: HIP events around every launch, a warm-up,
rounds of launches with the arms taken in turn, one process on one box.

Workload: the burst of docs/COHERENT_DEDISPERSION.md section 7 at n_int = 8 -- 4096 rows x 4 beams x 256 channels of Stokes cells
(64 MiB) -- on 512 Faraday depths.

  (a)   bf_rm_device, peaks only
  (a')  bf_rm_device, spectrum and peaks
  (b)   the same result as separate torch operations: gather Q + iU from the cells, complex64 matmul with the table, abs^2, argmax
  (c)   a device-to-device copy of the input

  python tools/rm_time.py [--rounds R] [--reps N]

The bar: median (a) <= median (b), in the same run; (a) / (c) and the largest |difference| between (a') and (b) are reported."""
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

    n_rows, K, n_chan, n_phi = 4096, 4, 256, 512
    bf = bfm.Beamformer(bfm.debug_config())
    freq = [host.channel_frequency(0, ch) for ch in range(n_chan)]
    fwhm, _ = api.rm_resolution(freq, None)
    rot, wn, _ = api.rm_table(freq, None, -256 * fwhm / 8, fwhm / 8, n_phi)
    stage = api.FaradaySynthesis(bf, n_chan, n_phi, rot, wn)
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((n_rows, n_chan, K, 4), generator=gen, device="cuda", dtype=torch.float32)
    nbytes = x.numel() * 4
    d_copy = torch.empty_like(x)
    d_spec = torch.zeros((n_rows, K, n_phi), dtype=torch.complex64, device="cuda")
    d_peaks = torch.zeros((n_rows, K, 8), dtype=torch.int32, device="cuda")
    d_peaks2 = torch.zeros_like(d_peaks)
    d_rot = torch.from_numpy(np.ascontiguousarray(rot.T)).cuda()                 # [chan][depth]

    def torch_arm():
        with torch.cuda.stream(stream):
            z = torch.complex(x[..., 1], x[..., 2]).permute(0, 2, 1).reshape(n_rows * K, n_chan)
            f = z @ d_rot
            p = f.real * f.real + f.imag * f.imag
            return f, p, p.argmax(dim=1)

    runs = {
        "a_rm_peaks_only": lambda: stage.run(x, K, n_rows, peaks=d_peaks, stream=stream.cuda_stream),
        "a1_rm_spectrum_and_peaks": lambda: stage.run(x, K, n_rows, spec=d_spec, peaks=d_peaks2, stream=stream.cuda_stream),
        "b_torch_separate_operations": torch_arm,
        "c_copy_of_the_input": lambda: hip.hipMemcpyAsync(C.c_void_p(d_copy.data_ptr()), C.c_void_p(x.data_ptr()), C.c_size_t(nbytes), 3,
                                                         C.c_void_p(stream.cuda_stream)),
    }
    f, p, at = torch_arm()
    runs["a1_rm_spectrum_and_peaks"]()
    runs["a_rm_peaks_only"]()
    stream.synchronize()
    res["largest_difference_from_torch"] = float((f.reshape(n_rows, K, n_phi) - d_spec).abs().max())
    res["largest_modulus"] = float(d_spec.abs().max())
    res["peaks_that_differ_from_torch_argmax"] = int((at.reshape(n_rows, K) != d_peaks2[..., 0]).sum())
    res["peak_records_equal_between_a_and_a1"] = bool(torch.equal(d_peaks, d_peaks2))
    del f, p, at

    t = {k: [] for k in runs}
    for fn in runs.values():
        timed(fn, 3)
    for _ in range(a.rounds):
        for k, fn in runs.items():
            t[k] += timed(fn, a.reps)
    print("%d rows x %d beams x %d channels on %d depths: %d rounds x %d launches, %.0f MiB of input" % (n_rows, K, n_chan, n_phi, a.rounds, a.reps, nbytes / 2 ** 20))
    flop = 8.0 * n_rows * K * n_chan * n_phi
    for k, v in t.items():
        v = sorted(v)
        res[k] = {"median_us": 1e3 * v[len(v) // 2], "min_us": 1e3 * v[0], "max_us": 1e3 * v[-1], "n": len(v)}
        print("  %-28s median %9.1f us   min %9.1f   max %9.1f   (%d)   %6.1f TFLOP/s of the product at the median"
              % (k, res[k]["median_us"], res[k]["min_us"], res[k]["max_us"], len(v), flop / res[k]["median_us"] / 1e6))
    am, bm, cm = (res[k]["median_us"] for k in ("a_rm_peaks_only", "b_torch_separate_operations", "c_copy_of_the_input"))
    res["a_over_c"] = am / cm
    res["bar_a_le_b"] = bool(am <= bm)
    print("  (a) / (c) = %.2f" % res["a_over_c"])
    print("  (a) <= (b): %.1f <= %.1f  %s" % (am, bm, "met" if res["bar_a_le_b"] else "MISSED"))
    stage.close()
    bf.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
