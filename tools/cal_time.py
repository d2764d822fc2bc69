#!/usr/bin/env python3
"""Times of the gain solver (docs/CALIBRATION.md) at C3 (64 antennas, 256 channels, 2 polarisations: 512 problems) and at 256 antennas,
on a synthetic calibrator field (V = rint(2^20 g g^H) + integer noise, |g| in 0.5 ... 1.5, random phases), tol 1e-10 -- HIP events
around every launch, a warm-up, the measurements taken in turn over three rounds of eight launches, in one process on one box:

  (a)  bf_solve_gains_device, every (channel, polarisation) on its own
  (b)  bf_calibrate_weights_device over the weight array, against (b0) a device-to-device copy of that array
  (c)  one bf_correlate_device launch over a block of 128 gemm-units

  python tools/cal_time.py [--rounds R] [--reps N] [--units U]

The bar of docs/CALIBRATION.md: (a) <= (c) at C3 -- a solve that costs more than the integration it follows would stall a pipeline
that dumps every block; (b) / (b0) is reported."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def calibrator_field(rng, n_ant, n_freq, n_pol, noise=200):
    """int64 [freq][pol][bl][2]: one point source at the phase centre seen through random gains, plus integer noise."""
    amp = rng.uniform(0.5, 1.5, size=(n_freq, n_pol, n_ant))
    g = amp * np.exp(2j * np.pi * rng.uniform(size=amp.shape))
    a1, a2 = np.tril_indices(n_ant)
    v = 2.0 ** 20 * g[..., a1] * np.conj(g[..., a2])
    vis = np.stack([np.rint(v.real), np.rint(v.imag)], axis=-1).astype(np.int64) + rng.integers(-noise, noise + 1, size=v.shape + (2,))
    vis[..., a1 == a2, 1] = 0
    return np.ascontiguousarray(vis)                   # (the fancy indexing above leaves another memory order)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--units", type=int, default=128)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    import dsabeamformer_amd as bfm
    from dsabeamformer_amd import _lib

    hip = _lib._preload_hip_runtime()
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(20261018)
    res = {"device": torch.cuda.get_device_name(0), "units": a.units}
    for label, cfg in (("c3", bfm.production_config(n_out_per_gemm=16)), ("a256", bfm.production_config(n_out_per_gemm=16, n_ant=256))):
        bf = bfm.Beamformer(cfg)
        d_vis_cal = torch.from_numpy(calibrator_field(rng, cfg.n_ant, cfg.n_freq, cfg.n_pol)).cuda()
        assert d_vis_cal.is_contiguous() and d_vis_cal.shape == (cfg.n_freq, cfg.n_pol, cfg.n_ant * (cfg.n_ant + 1) // 2, 2)
        d_gains = torch.zeros((cfg.n_pol, cfg.n_freq, cfg.n_ant, 2), dtype=torch.float64, device="cuda")
        d_info = torch.zeros((cfg.n_pol, cfg.n_freq, 2), dtype=torch.int32, device="cuda")
        d_w = torch.randint(-127, 128, (cfg.n_freq, cfg.n_ant, cfg.n_beams, 2), dtype=torch.int8, device="cuda")
        d_w_out = torch.empty_like(d_w)
        nbytes = bf.bytes_per_gemm * a.units
        d_in = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
        d_vis = torch.zeros(bf.corr_entries * 2, dtype=torch.int64, device="cuda")

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
            "a_solve_gains": lambda: bf.solve_gains(d_vis_cal, d_gains, d_info, stream=stream.cuda_stream),
            "b_calibrate_weights": lambda: bf.calibrate_weights(d_w, d_gains[0], d_w_out, stream=stream.cuda_stream),
            "b0_copy_of_the_weights": lambda: hip.hipMemcpyAsync(C.c_void_p(d_w_out.data_ptr()), C.c_void_p(d_w.data_ptr()), C.c_size_t(d_w.numel()),
                                                                 3, C.c_void_p(stream.cuda_stream)),
            "c_correlate_block": lambda: bf.correlate(d_in, a.units, d_vis, False, stream.cuda_stream),
        }
        t = {k: [] for k in runs}
        for fn in runs.values():                       # warm-up: every kernel and the copy
            timed(fn, 3)
        for _ in range(a.rounds):
            for k, fn in runs.items():
                t[k] += timed(fn, a.reps)
        info = d_info.cpu().numpy()
        its = info[..., 0]
        print("%s: %d antennas, %d problems, iterations %d ... %d (mean %.1f), %d of %d converged; %d MiB of weights; correlator input %d gemm-units, "
              "%.0f MiB; %d rounds x %d launches" % (label, cfg.n_ant, its.size, its.min(), its.max(), its.mean(), int((info[..., 1] == 1).sum()), its.size,
                                                   d_w.numel() >> 20, a.units, nbytes / 2 ** 20, a.rounds, a.reps))
        r = {"iterations_min": int(its.min()), "iterations_max": int(its.max()), "iterations_mean": float(its.mean()),
             "converged": int((info[..., 1] == 1).sum()), "problems": int(its.size)}
        for k, v in t.items():
            v = sorted(v)
            r[k] = {"median_us": 1e3 * v[len(v) // 2], "min_us": 1e3 * v[0], "max_us": 1e3 * v[-1], "n": len(v)}
            print("  %-24s median %9.1f us   min %9.1f   max %9.1f   (%d)" % (k, r[k]["median_us"], r[k]["min_us"], r[k]["max_us"], len(v)))
        am, bm, b0m, cm = (r[k]["median_us"] for k in runs)
        r["us_per_iteration"] = am / its.max()
        r["b_over_b0"] = bm / b0m
        r["bar_a_le_c"] = bool(am <= cm)
        print("  (a) per iteration of the longest problem: %.2f us;   (b) / (b0) = %.2f;   bar (a) <= (c): %.1f <= %.1f  %s"
              % (r["us_per_iteration"], r["b_over_b0"], am, cm, ("met" if r["bar_a_le_c"] else "MISSED") if label == "c3" else "(no bar here)"))
        res[label] = r
        bf.close()
        del d_in, d_vis, d_vis_cal, d_w, d_w_out, d_gains, d_info
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
