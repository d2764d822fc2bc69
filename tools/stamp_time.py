#!/usr/bin/env python3
"""Times of the stamp cut beside the DM push at the production DM shape (tools/sps_time.py's stage: 64 trials, pushes of 512 rows of
256 channels x 256 beams), HIP events, one process, a warm-up, then rounds with the arms taken in turn:

  (a)  a DM push on the parent commit's library    [--parent-lib LIB, through DSABF_LIB_PATH, in a subprocess per round]
  (a0) a DM push with this build, history_rows 0 (the parent's ring), no cut ever issued: the unarmed wait alone -- in a subprocess
       per round exactly as (a), so the two differ in the library and in nothing else
  (a') a DM push with this build, a stage with history on which no cut is ever issued: the larger ring as well
  (b)  one cut of 16 stamps, 256 channels x 64 bins, tbin 4, fbin 1
  (c)  the same cut queued on another queue between two pushes: the cut's time and the pushes' beside it

  python tools/stamp_time.py [--rounds R] [--pushes N] [--parent-lib variants/parent/libdsabf.so]
  python tools/stamp_time.py --host-only       # bf_evt_feed beside bf_sps_select on the same records: no GPU

The bars of docs/EVENTS.md: (a0) within (a)'s own min .. max; (b) <= median (a)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
N_DM, N_T, N_BEAMS, N_FREQ = 64, 512, 256, 256
N_STAMPS, BINS, TBIN, FBIN = 16, 64, 4, 1
N_BUF, MAX_WIDTH, T_TOL = 3, 32, 0


def history_rows():
    """docs/EVENTS.md section 3: half the stamp's span in front of the pulse, the wait for the cluster to close, the pushes in flight."""
    return BINS * TBIN // 2 + MAX_WIDTH + T_TOL + (N_BUF + 1) * N_T


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


def child_dm_only(a):
    """(a) on the library DSABF_LIB_PATH names: prints the times of one round as JSON."""
    torch, bfm, _lib, api, bf, delays = setup()
    hip = _lib._preload_hip_runtime()
    stream = torch.cuda.Stream()
    rows = torch.rand(N_T * N_FREQ * N_BEAMS, device="cuda")
    dm = api.DmStream(bf, delays, N_FREQ, N_T)
    time_dm_pushes(torch, hip, dm, rows, a.warm, stream)
    print(json.dumps(time_dm_pushes(torch, hip, dm, rows, a.pushes, stream)))


def host_side():
    """bf_evt_feed for the storm (a candidate in every (trial, beam)) and for a quiet push of 50 candidates, beside bf_sps_select on
    records that select exactly those candidates."""
    sys.path.insert(0, ROOT)
    import numpy as np

    from dsabeamformer_amd import api

    rng = np.random.default_rng(1)
    K = 6
    res = {}
    for name, n_hot in (("storm_16384", N_DM * N_BEAMS), ("quiet_50", 50)):
        value = np.zeros((K, N_DM, N_BEAMS), np.float32)
        t_end = np.full((K, N_DM, N_BEAMS), 100, np.int32)
        hot = rng.permutation(N_DM * N_BEAMS)[:n_hot]
        v2 = value[2].reshape(-1)
        v2[hot] = 40.0 + rng.random(n_hot)
        n = 4096
        sums, sumsq = np.zeros((N_DM, N_BEAMS)), np.full((N_DM, N_BEAMS), float(n))     # mu 0, sigma 1
        t_sel, t_feed = [], []
        for _ in range(9):
            t0 = time.perf_counter()
            cands = api.sps_select((value, t_end), (sums, sumsq), n, N_BEAMS, first_t=1000, threshold=8.0)
            t_sel.append(time.perf_counter() - t0)
            assert len(cands) == n_hot
            with api.EventBuilder(max_width=MAX_WIDTH, ib_beam=N_BEAMS - 1) as eb:
                t0 = time.perf_counter()
                ev = eb.feed(cands, 1000 + N_T)
                t_feed.append(time.perf_counter() - t0)
                n_events = len(ev) + len(eb.flush())
        res[name] = {"bf_sps_select_us": 1e6 * sorted(t_sel)[4], "bf_evt_feed_us": 1e6 * sorted(t_feed)[4], "events": n_events}
        print("  %-12s bf_sps_select %8.1f us   bf_evt_feed %8.1f us   (medians of 9, through the Python wrappers; %d events)"
              % (name, res[name]["bf_sps_select_us"], res[name]["bf_evt_feed_us"], n_events))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pushes", type=int, default=8)
    ap.add_argument("--warm", type=int, default=6)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child-dm-only", action="store_true")
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    if a.child_dm_only:
        return child_dm_only(a)
    if a.host_only:
        return host_side()
    torch, bfm, _lib, api, bf, delays = setup()
    import numpy as np

    hip = _lib._preload_hip_runtime()
    s_push, s_cut = torch.cuda.Stream(), torch.cuda.Stream()
    rows = torch.rand(N_T * N_FREQ * N_BEAMS, device="cuda")
    hist = history_rows()
    dm_cut = api.DmStream(bf, delays, N_FREQ, N_T, history_rows=hist)         # (a'): its pushes before the first cut; then (b), (c)
    cap = dm_cut.history()[2]
    assert cap >= int(np.max(delays)) + 3 * N_T + hist, "the stage did not get its ring (linear fallback)"
    d_out = torch.empty(N_STAMPS * (N_FREQ // FBIN) * BINS, device="cuda")
    t = {"a_dm_push_parent_lib": [], "a0_dm_push_history_0": [], "a1_dm_push_never_cut": [], "b_cut_16_stamps": [], "c_cut_between_pushes": [], "c_push_beside_the_cut": []}

    def requests():
        _, nxt, _ = dm_cut.history()
        out = []
        for k in range(N_STAMPS):
            d = (k * 4 + 3) % N_DM
            out.append((nxt - (BINS * TBIN + int(delays[d].max())) - 7 * k, d, (k * 37 + 5) % N_BEAMS))
        return out

    def cuts(n):
        out = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s_cut)
            st = dm_cut.cut(requests(), BINS, TBIN, FBIN, d_out, s_cut.cuda_stream)
            e1.record(s_cut)
            s_cut.synchronize()
            assert not st.any(), st
            out.append(e0.elapsed_time(e1))
        return out

    def cut_between_pushes(n):
        """push on one queue, the cut on another, the next push on the first: nothing waited for until all three are queued"""
        cut_t, push_t = [], []
        for _ in range(n):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            dst = dm_cut.reserve(N_T, s_push.cuda_stream)
            hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(rows.data_ptr()), C.c_size_t(rows.numel() * 4), 3, C.c_void_p(s_push.cuda_stream))
            ev[0].record(s_push)
            dm_cut.push(dst, N_T, None, s_push.cuda_stream)
            ev[1].record(s_push)
            ev[2].record(s_cut)
            st = dm_cut.cut(requests(), BINS, TBIN, FBIN, d_out, s_cut.cuda_stream)
            ev[3].record(s_cut)
            dst = dm_cut.reserve(N_T, s_push.cuda_stream)            # waits for the cut: it may overwrite what the cut reads
            hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(rows.data_ptr()), C.c_size_t(rows.numel() * 4), 3, C.c_void_p(s_push.cuda_stream))
            ev[4].record(s_push)
            dm_cut.push(dst, N_T, None, s_push.cuda_stream)
            ev[5].record(s_push)
            torch.cuda.synchronize()
            assert not st.any(), st
            cut_t.append(ev[2].elapsed_time(ev[3]))
            push_t += [ev[0].elapsed_time(ev[1]), ev[4].elapsed_time(ev[5])]
        return cut_t, push_t

    # warm-up: every kernel once, the delay windows and the history filled
    fill = (cap + N_T - 1) // N_T + 1
    time_dm_pushes(torch, hip, dm_cut, rows, max(a.warm, fill), s_push)
    # phase 1: the pushes, in turn, while no cut has ever been issued on any stage; phase 2: the cuts
    for r in range(a.rounds):
        for name, env in (("a_dm_push_parent_lib", dict(os.environ, DSABF_LIB_PATH=os.path.abspath(a.parent_lib)) if a.parent_lib else None),
                          ("a0_dm_push_history_0", dict(os.environ))):
            if env is None:
                continue
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-dm-only", "--pushes", str(a.pushes), "--warm", str(a.warm)],
                               env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:   # an abort, a fault or a time limit in the child: nothing more is started on this GPU
                print("%s: the child ended with status %d; stopping: %s" % (name, p.returncode, (p.stdout + p.stderr)[-600:]))
                sys.exit(1)
            t[name] += json.loads(p.stdout.strip().splitlines()[-1])
        t["a1_dm_push_never_cut"] += time_dm_pushes(torch, hip, dm_cut, rows, a.pushes, s_push)
    cuts(3)
    cut_between_pushes(2)
    for r in range(a.rounds):
        t["b_cut_16_stamps"] += cuts(a.pushes)
        c, p = cut_between_pushes(a.pushes // 2)
        t["c_cut_between_pushes"] += c
        t["c_push_beside_the_cut"] += p
    segs = sum(N_FREQ * (BINS * TBIN + int(delays[(k * 4 + 3) % N_DM].max())) for k in range(N_STAMPS))
    print("device: %s; %d rounds x %d; push = %d rows of %d x %d; ring %d rows (%.0f MiB), history_rows %d, max delay %d; cut = %d stamps x %d channels x "
          "%d bins, tbin %d: %d row segments"
          % (torch.cuda.get_device_name(0), a.rounds, a.pushes, N_T, N_FREQ, N_BEAMS, cap, cap * N_FREQ * N_BEAMS * 4 / 2 ** 20, hist, int(np.max(delays)),
             N_STAMPS, N_FREQ, BINS, TBIN, segs))
    res = {}
    if t["b_cut_16_stamps"]:
        b = t["b_cut_16_stamps"]
        print("  (b) slowest sample: %.1f us, number %d of its round of %d" % (1e3 * max(b), b.index(max(b)) % a.pushes, a.pushes))
    for name, v in t.items():
        if not v:
            continue
        v = sorted(v)
        res[name] = {"median_us": 1e3 * v[len(v) // 2], "min_us": 1e3 * v[0], "max_us": 1e3 * v[-1], "n": len(v)}
        print("  %-24s median %8.1f us   min %8.1f   max %8.1f   (n %d)" % (name, res[name]["median_us"], res[name]["min_us"], res[name]["max_us"], len(v)))
    if "a_dm_push_parent_lib" in res:
        pa, a1, b = res["a_dm_push_parent_lib"], res["a0_dm_push_history_0"], res["b_cut_16_stamps"]
        res["bar1_a0_within_a"] = bool(pa["min_us"] <= a1["min_us"] and a1["max_us"] <= pa["max_us"])
        ap_ = res["a1_dm_push_never_cut"]
        res["bar1_a1_within_a"] = bool(pa["min_us"] <= ap_["min_us"] and ap_["max_us"] <= pa["max_us"])   # the bar as stated: on (a')
        print("  bar 1 on (a'), the larger ring included: %s" % ("met" if res["bar1_a1_within_a"] else "MISSED"))
        res["bar2_b_le_a"] = bool(b["median_us"] <= pa["median_us"])
        print("  bar 1, (a0)'s min .. max within (a)'s: %s;  bar 2, (b) <= median (a): %s"
              % ("met" if res["bar1_a0_within_a"] else "MISSED", "met" if res["bar2_b_le_a"] else "MISSED"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
