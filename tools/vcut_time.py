#!/usr/bin/env python3
"""Times of the voltage cut and the voltage history's push at C3 (n_out_per_gemm 16: units of 8 MiB, 256 samples of 128 bytes x 256
channels) with 128 units resident, HIP events, one process, a warm-up, then rounds with the arms taken in turn:

  (a)  one cut of 4 requests x 2 units (64 MiB) at the production ladder's delays (64 trials, row delays x n_avg), beside a
       hipMemcpyAsync device-to-device of the same byte count; a matrix product is queued in front of either, so the host's
       time in the call is not between the events                                                   bar: median cut <= 1.5 x median copy
  (b)  bf_enqueue_block alone, and bf_enqueue_block + bf_vhist_push_block behind it on the same queue      reported, not barred
  (c)  with NO history created: a DM push and a block launch with this build and with the parent commit's library [--parent-lib LIB,
       through DSABF_LIB_PATH, a subprocess per round for both]                     bar: each median within the parent's own min .. max

  python tools/vcut_time.py [--rounds R] [--n N] [--parent-lib variants/parent/libdsabf.so]

docs/VOLTAGE_CUTS.md section 7 holds what this printed."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
N_DM, N_RESIDENT, N_REQ, CUT_UNITS = 64, 128, 4, 2
DM_ROWS = 512


def setup():
    sys.path.insert(0, ROOT)
    import torch

    import dsabeamformer_amd as bfm
    from dsabeamformer_amd import _lib, api, host

    cfg = bfm.production_config(n_out_per_gemm=16)
    bf = bfm.Beamformer(cfg)
    freq = [host.channel_frequency(0, c) for c in range(cfg.n_freq)]
    ladder = host.dm_trials(dm_max=250.0)
    dms = ladder[:: max(1, len(ladder) // N_DM)][:N_DM]
    delays = host.dm_delays(dms, freq, freq[0], 0.131)
    assert delays.shape == (N_DM, cfg.n_freq)
    return torch, bfm, _lib, api, host, bf, cfg, delays


def timed(torch, stream, fn, busy=None):
    """The event time of what fn queues on `stream`.  busy: a matrix whose product is queued first, so that the host has queued everything
    before the device reaches the first event -- the time between the events is then the device's alone, whatever the host spends in fn."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if busy is not None:
        with torch.cuda.stream(stream):
            torch.mm(busy, busy)
    a.record(stream)
    fn()
    b.record(stream)
    stream.synchronize()
    return a.elapsed_time(b)


def block_and_push_times(torch, bf, cfg, n, vh=None):
    """n block launches over the 32 units of ring slot 0 on compute queue 0 (+ the history's push behind each): event times in ms."""
    q = torch.cuda.ExternalStream(bf.queue_stream(0))
    n_u = cfg.n_gemms_per_block

    def one():
        bf.enqueue_block(0, 0, 0, n_u, None)
        if vh is not None:
            vh.push_block(0, 0, 0, n_u)
        bf.queue_stream(0)            # (launches what is still only queued)

    return [timed(torch, q, one) for _ in range(n)]


def dm_push_times(torch, hip, api, bf, cfg, delays, n, warm):
    stream = torch.cuda.Stream()
    rows = torch.rand(DM_ROWS * cfg.n_freq * cfg.n_beams, device="cuda")
    dm = api.DmStream(bf, delays, cfg.n_freq, DM_ROWS)
    out = []
    for k in range(warm + n):
        dst = dm.reserve(DM_ROWS, stream.cuda_stream)
        assert hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(rows.data_ptr()), C.c_size_t(rows.numel() * 4), 3, C.c_void_p(stream.cuda_stream)) == 0
        t = timed(torch, stream, lambda: dm.push(dst, DM_ROWS, None, stream.cuda_stream))
        if k >= warm:
            out.append(t)
    dm.close()
    return out


def load_block(torch, host, bf, cfg):
    import numpy as np

    rng = np.random.default_rng(1)
    bf.set_weights(host.make_weights_default(cfg.n_beams, cfg.n_ant, cfg.n_freq))
    block = torch.from_numpy(rng.integers(0, 256, size=cfg.n_gemms_per_block * cfg.n_freq * cfg.n_out_per_gemm * cfg.n_pol * cfg.n_avg * cfg.n_ant,
                                          dtype=np.uint8)).pin_memory()
    bf.submit_block(0, block, block.numel())
    bf.sync(-1)
    return block


def child_no_history(a):
    """(c) on the library DSABF_LIB_PATH names (or this build's): no history is created; prints one round's times as JSON."""
    torch, bfm, _lib, api, host, bf, cfg, delays = setup()
    hip = _lib._preload_hip_runtime()
    block = load_block(torch, host, bf, cfg)   # noqa: F841  (kept alive)
    block_and_push_times(torch, bf, cfg, a.warm)
    print(json.dumps({"block": block_and_push_times(torch, bf, cfg, a.n), "dm_push": dm_push_times(torch, hip, api, bf, cfg, delays, a.n, a.warm)}))


def summary(v):
    v = sorted(v)
    return {"median_us": 1e3 * v[len(v) // 2], "min_us": 1e3 * v[0], "max_us": 1e3 * v[-1], "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child-no-history", action="store_true")
    a = ap.parse_args()
    if a.child_no_history:
        return child_no_history(a)
    t = {"c_block_parent_lib": [], "c_dm_push_parent_lib": [], "c_block_this_build": [], "c_dm_push_this_build": []}
    # (c) first, before this process opens the device: a subprocess per round and arm, in turn
    for r in range(a.rounds):
        for name, env in (("parent_lib", dict(os.environ, DSABF_LIB_PATH=os.path.abspath(a.parent_lib)) if a.parent_lib else None),
                          ("this_build", dict(os.environ))):
            if env is None:
                continue
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-no-history", "--n", str(a.n), "--warm", str(a.warm)],
                               env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:   # an abort, a fault or a time limit in the child: nothing more is started on this GPU
                print("%s: the child ended with status %d; stopping: %s" % (name, p.returncode, (p.stdout + p.stderr)[-600:]))
                sys.exit(1)
            got = json.loads(p.stdout.strip().splitlines()[-1])
            t["c_block_" + name] += got["block"]
            t["c_dm_push_" + name] += got["dm_push"]
    torch, bfm, _lib, api, host, bf, cfg, delays = setup()
    hip = _lib._preload_hip_runtime()
    S, unit_bytes = cfg.n_out_per_gemm * cfg.n_avg, cfg.n_freq * cfg.n_out_per_gemm * cfg.n_avg * cfg.n_pol * cfg.n_ant
    block = load_block(torch, host, bf, cfg)   # noqa: F841
    vh = api.VoltageHistory(bf, delays * cfg.n_avg, N_RESIDENT)
    s_cut = torch.cuda.Stream()
    d_out = torch.empty(N_REQ * CUT_UNITS * unit_bytes, dtype=torch.uint8, device="cuda")
    d_src = torch.empty(N_REQ * CUT_UNITS * unit_bytes, dtype=torch.uint8, device="cuda").random_(0, 256)
    t.update({"a_cut_4x2_units": [], "a_copy_same_bytes": [], "b_block_alone": [], "b_block_and_history_push": []})

    def requests():
        _, nxt, _ = vh.history()
        out = []
        for k in range(N_REQ):
            d = (k * 16 + 15) % N_DM
            out.append((nxt * S - (CUT_UNITS * S + int(delays[d].max()) * cfg.n_avg) - 37 * k, d))
        return out

    busy = torch.randn((3072, 3072), device="cuda")   # a product of some hundred microseconds in front of both arms of (a)

    def cut():
        st = vh.cut(reqs, CUT_UNITS, d_out, s_cut.cuda_stream)
        assert not st.any(), st

    def copy():
        assert hip.hipMemcpyAsync(C.c_void_p(d_out.data_ptr()), C.c_void_p(d_src.data_ptr()), C.c_size_t(d_out.numel()), 3, C.c_void_p(s_cut.cuda_stream)) == 0

    # warm-up: the history filled (128 units: four pushes of the resident block), every kernel once
    for _ in range(N_RESIDENT // cfg.n_gemms_per_block + 1):
        vh.push_block(0, 0, 0, cfg.n_gemms_per_block)
    block_and_push_times(torch, bf, cfg, a.warm)
    block_and_push_times(torch, bf, cfg, a.warm, vh)
    reqs = requests()
    for _ in range(a.warm):
        timed(torch, s_cut, cut, busy)
        timed(torch, s_cut, copy, busy)
    torch.cuda.synchronize()
    for r in range(a.rounds):
        reqs = requests()                 # (the pushes of (b) have moved the newest sample)
        t["a_cut_4x2_units"] += [timed(torch, s_cut, cut, busy) for _ in range(a.n)]
        t["a_copy_same_bytes"] += [timed(torch, s_cut, copy, busy) for _ in range(a.n)]
        t["b_block_alone"] += block_and_push_times(torch, bf, cfg, a.n)
        t["b_block_and_history_push"] += block_and_push_times(torch, bf, cfg, a.n, vh)
    print("device: %s; %d rounds x %d; units of %d MiB (S %d, B %d, %d channels); history of %d units (%.0f MiB); cut = %d requests x %d units = %d MiB, "
          "largest delay %d samples" % (torch.cuda.get_device_name(0), a.rounds, a.n, unit_bytes >> 20, S, cfg.n_pol * cfg.n_ant, cfg.n_freq, N_RESIDENT,
                                        N_RESIDENT * unit_bytes / 2 ** 20, N_REQ, CUT_UNITS, d_out.numel() >> 20, int(delays.max()) * cfg.n_avg))
    res = {}
    for name, v in t.items():
        if v:
            res[name] = summary(v)
            print("  %-28s median %9.1f us   min %9.1f   max %9.1f   (n %d)" % (name, res[name]["median_us"], res[name]["min_us"], res[name]["max_us"], len(v)))
    ratio = res["a_cut_4x2_units"]["median_us"] / res["a_copy_same_bytes"]["median_us"]
    res["bar_a_cut_le_1p5_copy"] = bool(ratio <= 1.5)
    print("  bar (a): median cut / median copy = %.3f (<= 1.5): %s;  cut: %.2f TB/s read + written" % (
        ratio, "met" if res["bar_a_cut_le_1p5_copy"] else "MISSED", 2 * d_out.numel() / (res["a_cut_4x2_units"]["median_us"] * 1e-6) / 1e12))
    if t["c_block_parent_lib"]:
        for what in ("block", "dm_push"):
            pa, me = res["c_%s_parent_lib" % what], res["c_%s_this_build" % what]
            res["bar_c_%s_within_parent" % what] = bool(pa["min_us"] <= me["median_us"] <= pa["max_us"])
            print("  bar (c) %s: this build's median within the parent's min .. max: %s" % (what, "met" if res["bar_c_%s_within_parent" % what] else "MISSED"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
