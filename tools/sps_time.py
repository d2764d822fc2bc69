#!/usr/bin/env python3
"""Times of the single-pulse search stage at the production DM shape (64 trials x 512 times x 256 beams per push, widths 1 .. 32),
HIP events around every push, the four measurements taken in turn, round after round, in one process on one box:

  (a) a DM push with no search stage attached      [--parent-lib LIB: also on that library, in a subprocess per round]
  (b) a DM push with the stage attached
  (c) the search push alone, on a resident chunk
  (d) a device-to-device hipMemcpyAsync of the same 32 MiB chunk

  python tools/sps_time.py [--rounds R] [--pushes N] [--widths K] [--parent-lib variants/parent/libdsabf.so]

The bar of docs/SINGLE_PULSE.md: (c) <= 2 x (d).  The DM pushes take the zero-copy feed (bf_dm_stream_reserve); their rows are
written before the first event is recorded."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
N_DM, N_T, N_BEAMS, N_FREQ = 64, 512, 256, 256


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


def time_dm_pushes(torch, hip, dm, sps, rows, n, stream):
    """n pushes of N_T rows through `dm` (zero-copy feed); returns the event times in ms.  With a stage attached every push is
    collected after its queue has drained (outside the timed window)."""
    out = []
    for _ in range(n):
        dst = dm.reserve(N_T, stream.cuda_stream)
        assert hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(rows.data_ptr()), C.c_size_t(rows.numel() * 4), 3, C.c_void_p(stream.cuda_stream)) == 0
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        _, n_out = dm.push(dst, N_T, None, stream.cuda_stream)
        b.record(stream)
        stream.synchronize()
        if sps is not None and n_out:
            sps.collect()
        if n_out == N_T:            # (the first pushes fill the delay window: shorter chunks)
            out.append(a.elapsed_time(b))
    return out


def child_dm_only(a):
    """(a) on the library DSABF_LIB_PATH names: prints the times of one round as JSON."""
    torch, bfm, _lib, api, bf, delays = setup()
    hip = _lib._preload_hip_runtime()
    stream = torch.cuda.Stream()
    rows = torch.rand(N_T * N_FREQ * N_BEAMS, device="cuda")
    dm = api.DmStream(bf, delays, N_FREQ, N_T)
    time_dm_pushes(torch, hip, dm, None, rows, 4, stream)
    print(json.dumps(time_dm_pushes(torch, hip, dm, None, rows, a.pushes, stream)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pushes", type=int, default=8)
    ap.add_argument("--widths", type=int, default=6)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child-dm-only", action="store_true")
    a = ap.parse_args()
    if a.child_dm_only:
        return child_dm_only(a)
    torch, bfm, _lib, api, bf, delays = setup()
    hip = _lib._preload_hip_runtime()
    stream = torch.cuda.Stream()
    rows = torch.rand(N_T * N_FREQ * N_BEAMS, device="cuda")
    chunk = torch.rand(N_DM * N_T * N_BEAMS, device="cuda") * 1e3
    copy_dst = torch.empty_like(chunk)
    dm_plain = api.DmStream(bf, delays, N_FREQ, N_T)
    dm_search = api.DmStream(bf, delays, N_FREQ, N_T)
    sps_attached = api.SinglePulseSearch(bf, N_DM, a.widths, N_T)
    dm_search.attach_search(sps_attached)
    sps_alone = api.SinglePulseSearch(bf, N_DM, a.widths, N_T)
    t = {"a_dm_push": [], "b_dm_push_with_search": [], "c_search_push": [], "d_copy_32MiB": [], "a_dm_push_parent_lib": []}

    def search_alone(n, first_t):
        out = []
        for i in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            sps_alone.push(chunk, N_T, first_t + i * N_T, stream.cuda_stream)
            e1.record(stream)
            stream.synchronize()
            sps_alone.collect()
            out.append(e0.elapsed_time(e1))
        return out

    def copies(n):
        out = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert hip.hipMemcpyAsync(C.c_void_p(copy_dst.data_ptr()), C.c_void_p(chunk.data_ptr()), C.c_size_t(chunk.numel() * 4), 3,
                                      C.c_void_p(stream.cuda_stream)) == 0
            e1.record(stream)
            stream.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    # warm-up: every kernel and copy once, the delay windows filled
    time_dm_pushes(torch, hip, dm_plain, None, rows, 4, stream)
    time_dm_pushes(torch, hip, dm_search, sps_attached, rows, 4, stream)
    search_alone(4, 0)
    copies(4)
    for r in range(a.rounds):
        t["a_dm_push"] += time_dm_pushes(torch, hip, dm_plain, None, rows, a.pushes, stream)
        t["b_dm_push_with_search"] += time_dm_pushes(torch, hip, dm_search, sps_attached, rows, a.pushes, stream)
        t["c_search_push"] += search_alone(a.pushes, (4 + r * a.pushes) * N_T)
        t["d_copy_32MiB"] += copies(a.pushes)
        if a.parent_lib:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-dm-only", "--pushes", str(a.pushes)],
                               env=dict(os.environ, DSABF_LIB_PATH=os.path.abspath(a.parent_lib)), capture_output=True, text=True, timeout=600)
            try:
                t["a_dm_push_parent_lib"] += json.loads(p.stdout.strip().splitlines()[-1])
            except Exception:
                print("parent-lib round failed: %s" % (p.stdout + p.stderr)[-600:])
    print("device: %s; %d rounds x %d pushes; push = %d trials x %d times x %d beams (%.0f MiB), widths 1 .. %d"
          % (torch.cuda.get_device_name(0), a.rounds, a.pushes, N_DM, N_T, N_BEAMS, N_DM * N_T * N_BEAMS * 4 / 2 ** 20, 1 << (a.widths - 1)))
    res = {}
    for name, v in t.items():
        if not v:
            continue
        v = sorted(v)
        res[name] = {"median_us": 1e3 * v[len(v) // 2], "min_us": 1e3 * v[0], "max_us": 1e3 * v[-1], "n": len(v)}
        print("  %-24s median %8.1f us   min %8.1f   max %8.1f   (%d pushes)" % (name, res[name]["median_us"], res[name]["min_us"], res[name]["max_us"], len(v)))
    c, d = res["c_search_push"]["median_us"], res["d_copy_32MiB"]["median_us"]
    res["bar_c_le_2d"] = bool(c <= 2 * d)
    print("  bar (c) <= 2 x (d): %.1f <= %.1f  %s" % (c, 2 * d, "met" if res["bar_c_le_2d"] else "MISSED"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
