#!/usr/bin/env python3
"""Times of the spatial null (docs/NULLING.md) at C3 (64 antennas, 256 channels, 2 polarisations, 256 beams) on the scene of
tests/test_gpu_null.py -- one interferer at amplitude 2 against unit noise as 4-bit voltages, 4096 columns per polarisation, here in a
quarter of the channels -- HIP events around every launch, a warm-up, the measurements taken in turn over three rounds of eight
launches, in one process on one box:

  (a)   bf_null_solve_device, n_null = 2
  (b)   bf_null_weights_device (BF_NULL_SCALED) over the weight array, with the vectors of (a)
  (b0)  bf_calibrate_weights_device on the same weights
  (c)   one bf_correlate_device launch over a block of 128 gemm-units

  python tools/null_time.py [--rounds R] [--reps N] [--units U]

The bar of docs/NULLING.md: (a) <= (c) -- a solve per dump must not cost more than the launch that produces its input; (b) / (b0) is
reported."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def scene_visibilities(n_ant, n_freq, n_pol, columns, every=4, seed=20261019):
    """int64 [freq][pol][bl][2], C-contiguous: the visibilities of 4-bit voltages v = 2 s x + n (|s_a| = 1, x and n unit complex
    Gaussians) in the channels f = 0 (mod every) and of the noise alone elsewhere.  numpy on the host, so that every run times the same
    field; float64 products of integers below 2^53: exact."""
    rng = np.random.default_rng(seed)
    rn = lambda *shape: rng.standard_normal(shape) * 0.5 ** 0.5   # noqa: E731
    a1, a2 = np.tril_indices(n_ant)
    vis = np.empty((n_freq, n_pol, a1.size, 2), np.int64)
    step = 16
    for f0 in range(0, n_freq, step):
        on = (np.arange(f0, f0 + step) % every == 0).astype(np.float64)[:, None, None, None]
        ph = 2 * np.pi * rng.uniform(size=(step, 1, 1, n_ant))
        xr, xi = rn(step, n_pol, columns, 1), rn(step, n_pol, columns, 1)
        vr = 2 * on * (np.cos(ph) * xr - np.sin(ph) * xi) + rn(step, n_pol, columns, n_ant)
        vi = 2 * on * (np.cos(ph) * xi + np.sin(ph) * xr) + rn(step, n_pol, columns, n_ant)
        vr, vi = np.clip(np.rint(vr), -8, 7), np.clip(np.rint(vi), -8, 7)
        vrt, vit = vr.transpose(0, 1, 3, 2), vi.transpose(0, 1, 3, 2)
        re = vrt @ vr + vit @ vi                                              # V[a1][a2] = sum v[a1] conj(v[a2])
        im = vit @ vr - vrt @ vi
        vis[f0:f0 + step, :, :, 0] = re[..., a1, a2]
        vis[f0:f0 + step, :, :, 1] = im[..., a1, a2]
    assert np.all(vis[:, :, a1 == a2, 0] > 0) and not vis[:, :, a1 == a2, 1].any()
    return np.ascontiguousarray(vis)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--units", type=int, default=128)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    import dsabeamformer_amd as bfm

    n_null = 2
    cfg = bfm.production_config(n_out_per_gemm=16)
    bf = bfm.Beamformer(cfg)
    scene = scene_visibilities(cfg.n_ant, cfg.n_freq, cfg.n_pol, 4096)
    d_vis_scene = torch.from_numpy(scene).cuda()
    assert d_vis_scene.is_contiguous() and d_vis_scene.shape == (cfg.n_freq, cfg.n_pol, cfg.n_ant * (cfg.n_ant + 1) // 2, 2)
    d_vecs = torch.zeros((cfg.n_freq, n_null, cfg.n_ant, 2), dtype=torch.float64, device="cuda")
    d_eig = torch.zeros((cfg.n_freq, n_null + 1), dtype=torch.float64, device="cuda")
    d_info = torch.zeros((cfg.n_freq, 1 + 2 * n_null), dtype=torch.int32, device="cuda")
    d_scale = torch.zeros((cfg.n_freq,), dtype=torch.float64, device="cuda")
    d_gains = torch.zeros((cfg.n_freq, cfg.n_ant, 2), dtype=torch.float64, device="cuda")
    d_gains[..., 0] = 1.0
    d_w = torch.randint(-127, 128, (cfg.n_freq, cfg.n_ant, cfg.n_beams, 2), dtype=torch.int8, device="cuda")
    d_w_out = torch.empty_like(d_w)
    nbytes = bf.bytes_per_gemm * a.units
    d_in = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
    d_vis = torch.zeros(bf.corr_entries * 2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()                           # everything above ran on the default stream; the launches below use one of their own
    stream = torch.cuda.Stream()

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
        "a_null_solve": lambda: bf.null_solve(d_vis_scene, d_vecs, d_eig, d_info, n_null=n_null, stream=stream.cuda_stream),
        "b_null_weights": lambda: bf.null_weights(d_w, d_vecs, d_info, d_w_out, n_null, scale=d_scale, stream=stream.cuda_stream),
        "b0_calibrate_weights": lambda: bf.calibrate_weights(d_w, d_gains, d_w_out, stream=stream.cuda_stream),
        "c_correlate_block": lambda: bf.correlate(d_in, a.units, d_vis, False, stream.cuda_stream),
    }
    t = {k: [] for k in runs}
    for fn in runs.values():                           # warm-up: every kernel
        timed(fn, 3)
    for _ in range(a.rounds):
        for k, fn in runs.items():
            t[k] += timed(fn, a.reps)
    info = d_info.cpu().numpy()
    # what was timed is what the contract says: the last solve against the numpy restatement, to the bit (the calibration tool once timed a
    # field that had reached the device in another memory order, docs/CALIBRATION.md section 6)
    sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
    import null_oracle

    want = null_oracle.solve(scene, cfg.n_ant, n_null=n_null)
    equal = bool(np.array_equal(info, want[2]) and np.array_equal(d_vecs.cpu().numpy().view(np.int64), want[0].view(np.int64))
                 and np.array_equal(d_eig.cpu().numpy().view(np.int64), want[1].view(np.int64)))
    print("the last solve equals tests/support/null_oracle.py to the bit: %s" % equal)
    res = {"equals_oracle": equal, "device": torch.cuda.get_device_name(0), "units": a.units, "n_ant": cfg.n_ant, "n_freq": cfg.n_freq, "n_beams": cfg.n_beams,
           "n_null": n_null, "n_used_histogram": np.bincount(info[:, 0], minlength=n_null + 1).tolist()}
    print("C3: %d antennas, %d channels, %d beams; n_used histogram %s; %d MiB of weights; correlator input %d gemm-units, %.0f MiB; %d rounds x %d launches"
          % (cfg.n_ant, cfg.n_freq, cfg.n_beams, res["n_used_histogram"], d_w.numel() >> 20, a.units, nbytes / 2 ** 20, a.rounds, a.reps))
    for j in range(n_null):
        its, st = info[:, 1 + 2 * j], info[:, 2 + 2 * j]
        res["vector_%d" % j] = {"iterations_min": int(its.min()), "iterations_max": int(its.max()), "iterations_mean": float(its.mean()),
                                "converged": int((st == 1).sum()), "ran_out": int((st == 0).sum()), "nothing_left": int((st == 2).sum())}
        print("  vector %d: iterations %d ... %d (mean %.1f), %d converged, %d ran out, %d had nothing left"
              % (j, its.min(), its.max(), its.mean(), (st == 1).sum(), (st == 0).sum(), (st == 2).sum()))
    for k, v in t.items():
        v = sorted(v)
        res[k] = {"median_us": 1e3 * v[len(v) // 2], "min_us": 1e3 * v[0], "max_us": 1e3 * v[-1], "n": len(v)}
        print("  %-24s median %9.1f us   min %9.1f   max %9.1f   (%d)" % (k, res[k]["median_us"], res[k]["min_us"], res[k]["max_us"], len(v)))
    am, bm, b0m, cm = (res[k]["median_us"] for k in runs)
    longest = int(info[:, 1::2].sum(axis=1).max())
    res["us_per_multiplication"] = am / max(longest, 1)
    res["b_over_b0"] = bm / b0m
    res["bar_a_le_c"] = bool(am <= cm)
    print("  (a) per multiplication of the longest channel (%d): %.2f us;   (b) / (b0) = %.2f;   bar (a) <= (c): %.1f <= %.1f  %s"
          % (longest, res["us_per_multiplication"], res["b_over_b0"], am, cm, "met" if res["bar_a_le_c"] else "MISSED"))
    bf.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
