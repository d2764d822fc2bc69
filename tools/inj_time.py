#!/usr/bin/env python3
"""Times of the pulse injector beside the DM push at the production DM shape (tools/sps_time.py's stage: 64 trials, pushes of 512 rows of
256 channels x 256 beams), HIP events, one process, a warm-up, then rounds with the arms taken in turn:

  (a)  a DM push on the parent commit's library    [--parent-lib LIB, through DSABF_LIB_PATH, in a subprocess per round]
  (a') a DM push with this build and an attached, idle injector -- in a subprocess per round exactly as (a); structural, not barred:
       an idle apply launches nothing (tests/test_gpu_inj.py), the two medians are reported side by side
  (b)  an apply with one burst of 64 rows in one beam, swept over the band (delay[f] = f): the rows it touches, read and written
  (c)  an apply with one train over the whole push; the same with four trains
  (d)  hipMemcpyAsync, device to device, of the same rows
  (e)  bf_cond_push on the same rows

  python tools/inj_time.py [--rounds R] [--pushes N] [--parent-lib variants/parent/libdsabf.so]

The bar of docs/INJECTION.md: (c) with one train <= (e), medians of the same run.  (c) / (d) and the four-train figure are reported."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
N_DM, N_T, N_BEAMS, N_FREQ = 64, 512, 256, 256
BURST_W, BURST_T0, N_BINS = 64, 100, 64


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


def child_dm(a):
    """(a) / (a') on the library DSABF_LIB_PATH names (none: this build): prints the times of one round as JSON."""
    torch, bfm, _lib, api, bf, delays = setup()
    hip = _lib._preload_hip_runtime()
    stream = torch.cuda.Stream()
    rows = torch.rand(N_T * N_FREQ * N_BEAMS, device="cuda")
    dm = api.DmStream(bf, delays, N_FREQ, N_T)
    inj = None
    if a.child_dm == "idle":
        inj = api.Injector(bf, N_FREQ, N_T)
        dm.attach_injector(inj)
    time_dm_pushes(torch, hip, dm, rows, a.warm, stream)
    out = time_dm_pushes(torch, hip, dm, rows, a.pushes, stream)
    assert inj is None or (inj.launches == 0 and inj.next_row == (a.warm + a.pushes) * N_T)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pushes", type=int, default=8)
    ap.add_argument("--warm", type=int, default=6)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child-dm", choices=("plain", "idle"), default=None)
    a = ap.parse_args()
    if a.child_dm:
        return child_dm(a)
    torch, bfm, _lib, api, bf, delays = setup()
    import numpy as np

    hip = _lib._preload_hip_runtime()
    st = torch.cuda.Stream()
    rows = torch.rand(N_T * N_FREQ * N_BEAMS, device="cuda")
    rows2 = torch.empty_like(rows)
    resp = np.zeros(N_BEAMS, np.float32)
    resp[3] = 1.0
    sweep = np.arange(N_FREQ, dtype=np.int32)                                  # the burst crosses the band in 256 rows: 100 .. 418 of the push
    assert BURST_T0 + N_FREQ - 1 + BURST_W <= N_T
    burst_prof = api.Injector.burst_profile(N_FREQ, BURST_W, (BURST_W - 1) / 2.0, 4.0, 1.0)
    train_prof = np.zeros((N_FREQ, N_BINS), np.float32)
    train_prof[:, :3] = 0.1
    trial = delays[N_DM // 2]

    def timed(fn, n):
        out = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn()
            e1.record(st)
            st.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    inj_b = api.Injector(bf, N_FREQ, N_T, max_width=BURST_W)

    def burst_apply():
        inj_b.apply(rows, N_T, st.cuda_stream)

    def bursts(n):
        out = []
        for _ in range(n):
            inj_b.add_burst(inj_b.next_row + BURST_T0, sweep, burst_prof, resp)   # (outside the events: an add is host work and one small copy)
            before = inj_b.launches
            out += timed(burst_apply, 1)
            assert inj_b.launches == before + 1
        return out

    def train_stage(n_trains):
        s = api.Injector(bf, N_FREQ, N_T, max_width=N_BINS)
        for k in range(n_trains):
            s.add_train(api.PulsarFolder.model_from_spin(3.3 + k, row_seconds=0.131e-3), trial, train_prof, resp)
        return s

    inj_1, inj_4 = train_stage(1), train_stage(4)
    cond = api.Conditioner(bf, N_FREQ, N_T)
    arms = {"b_apply_one_burst_64_rows": bursts,
            "c_apply_one_train": lambda n: timed(lambda: inj_1.apply(rows, N_T, st.cuda_stream), n),
            "c_apply_four_trains": lambda n: timed(lambda: inj_4.apply(rows, N_T, st.cuda_stream), n),
            "d_memcpy_device_to_device": lambda n: timed(lambda: hip.hipMemcpyAsync(C.c_void_p(rows2.data_ptr()), C.c_void_p(rows.data_ptr()),
                                                                                    C.c_size_t(rows.numel() * 4), 3, C.c_void_p(st.cuda_stream)), n),
            "e_bf_cond_push": lambda n: timed(lambda: cond.push(rows, N_T, st.cuda_stream), n)}
    t = {"a_dm_push_parent_lib": [], "a1_dm_push_idle_injector": []}
    t.update({k: [] for k in arms})
    for fn in arms.values():                       # warm-up: every kernel once and more
        fn(a.warm)
    for r in range(a.rounds):
        for name, env, mode in (("a_dm_push_parent_lib", dict(os.environ, DSABF_LIB_PATH=os.path.abspath(a.parent_lib)) if a.parent_lib else None, "plain"),
                                ("a1_dm_push_idle_injector", dict(os.environ), "idle")):
            if env is None:
                continue
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-dm", mode, "--pushes", str(a.pushes), "--warm", str(a.warm)],
                               env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:   # an abort, a fault or a time limit in the child: nothing more is started on this GPU
                print("%s: the child ended with status %d; stopping: %s" % (name, p.returncode, (p.stdout + p.stderr)[-600:]))
                sys.exit(1)
            t[name] += json.loads(p.stdout.strip().splitlines()[-1])
        for name, fn in arms.items():
            t[name] += fn(a.pushes)
    push_bytes = N_T * N_FREQ * N_BEAMS * 4
    burst_bytes = 2 * BURST_W * N_FREQ * N_BEAMS * 4
    print("device: %s; %d rounds x %d; push = %d rows of %d x %d (%.0f MiB); burst = %d rows per channel, %.1f MiB read + written"
          % (torch.cuda.get_device_name(0), a.rounds, a.pushes, N_T, N_FREQ, N_BEAMS, push_bytes / 2 ** 20, BURST_W, burst_bytes / 2 ** 20))
    res = {}
    for name, v in t.items():
        if not v:
            continue
        v = sorted(v)
        res[name] = {"median_us": 1e3 * v[len(v) // 2], "min_us": 1e3 * v[0], "max_us": 1e3 * v[-1], "n": len(v)}
        print("  %-28s median %8.1f us   min %8.1f   max %8.1f   (n %d)" % (name, res[name]["median_us"], res[name]["min_us"], res[name]["max_us"], len(v)))
    c1, c4, d, e, b = (res[k]["median_us"] for k in ("c_apply_one_train", "c_apply_four_trains", "d_memcpy_device_to_device", "e_bf_cond_push",
                                                     "b_apply_one_burst_64_rows"))
    res["c_over_d"], res["c4_over_c1"] = c1 / d, c4 / c1
    res["c_tb_per_s"], res["b_tb_per_s"] = 2 * push_bytes / c1 / 1e6, burst_bytes / b / 1e6
    res["bar_c_le_e"] = bool(c1 <= e)
    print("  (c) / (d) = %.2f; four trains / one = %.2f; (c) moves %.2f TB/s, (b) %.2f TB/s of the rows it touches" % (res["c_over_d"], res["c4_over_c1"],
                                                                                                              res["c_tb_per_s"], res["b_tb_per_s"]))
    print("  bar, (c) one train <= (e) bf_cond_push: %s" % ("met" if res["bar_c_le_e"] else "MISSED"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
