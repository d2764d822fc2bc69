"""GPU tests (-m gpu) of the multi-rank paths with MORE THAN ONE RANK -- on one GPU.  RCCL refuses two ranks on one
device and the pool has 1-GPU boxes, so the ranks (separate processes, as in production: one process per shard) time-share
GPU 0 and their point-to-point messages travel through tests/support/fake_rccl.cpp, a loopback stand-in for the eight
RCCL entry points csrc/bf_comm.cpp binds (selected with DSABF_RCCL_LIB; same matching rules: per-pair issue order,
concurrent progress inside a group, sizes must agree).  Everything else is the product: bf_comm_create,
bf_gather_detected's plan walk and grouping, `beam -R world -r rank`, the gather inside run_observation."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, sweep

pytestmark = pytest.mark.gpu
SUPPORT = os.path.join(ROOT, "tests", "support")
FAKE = os.path.join(SUPPORT, "libfakerccl.so")


@pytest.fixture(scope="module")
def fake_rccl():
    """Builds the loopback stand-in (no DT_NEEDED on a HIP runtime: it binds to the one already in the process)."""
    src = os.path.join(SUPPORT, "fake_rccl.cpp")
    if not os.path.exists(FAKE) or os.path.getmtime(FAKE) < os.path.getmtime(src):
        from dsabeamformer_amd import build

        obj = os.path.join(SUPPORT, "fake_rccl.o")
        subprocess.check_call([build.HIPCC, "-O2", "-std=c++17", "-fPIC", "-c", src, "-o", obj])
        cxx = os.path.join(os.path.dirname(os.path.realpath(build.HIPCC)), "..", "lib", "llvm", "bin", "clang++")
        subprocess.check_call([cxx if os.path.exists(cxx) else "g++", "-shared", "-fPIC", "-o", FAKE, obj, "-lpthread", "-lrt"])
    return FAKE


@pytest.mark.parametrize("world", sweep([2, 4, 8], [4]))     # (8 ranks: the true config-4 shape below, always)
def test_gather_detected_with_several_ranks_on_one_gpu(orc, fake_rccl, tmp_path, world):
    # 8 ranks = BASELINE configs[3]'s partition (one process per GPU there; here they time-share GPU 0)
    env = dict(os.environ, DSABF_RCCL_LIB=fake_rccl, FAKERCCL_MAILBOX_MB="2" if world == 8 else "16")
    rng = np.random.default_rng(5)
    delays = np.sort(rng.integers(0, 3, size=(3, 8 * world)), axis=1)[:, ::-1].astype(np.int32).copy()   # [dm][F], falling with f
    delays[0] = 0
    np.save(tmp_path / "delays.npy", delays)
    procs = [subprocess.Popen([sys.executable, os.path.join(SUPPORT, "gather_worker.py"), str(r), str(world), str(tmp_path)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    prob = np.load(tmp_path / "problem.npz")
    w, packed = prob["w"], prob["packed"]
    F, B = w.shape[0], w.shape[2]
    fl = F // world
    g = orc.Geom(n_beams=B, n_ant=64, n_freq=F, n_avg=16, n_out_per_gemm=2)
    want = orc.beamform(g, w, packed)                              # [unit][o][F][b]: the whole band
    n_rows = want.shape[0] * want.shape[1]
    full = want.reshape(n_rows, F, B)
    ranks = [np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world)]
    for r in range(world):                                          # every shard's own kernel output
        assert np.array_equal(ranks[r]["local"].reshape(n_rows, fl, B), full[:, r * fl:(r + 1) * fl])
    shards = np.stack([full[:, r * fl:(r + 1) * fl] for r in range(world)])      # [rank][row][f_local][b]
    for root in (0, world - 1, -1, -2):
        receivers = [root] if root >= 0 else list(range(world))
        for r in range(world):
            keys = [k for k in ranks[r].files if k.startswith("root%d_" % root)]
            assert bool(keys) == (r in receivers), (root, r, keys)
        for r in receivers:
            held = n_rows // world if root == -2 else n_rows
            first = r * held if root == -2 else 0
            got_f = ranks[r]["root%d_layout0" % root].reshape(held, F, B)          # the reference's [o][f][b]
            got_r = ranks[r]["root%d_layout1" % root].reshape(world, held, fl, B)  # sub-band-major
            assert np.array_equal(got_f, full[first:first + held]), (root, r)
            assert np.array_equal(got_r, shards[:, first:first + held]), (root, r)
            # the staged transport (one message per sender + the device re-layout pass): the same [o][f][b], bit for bit
            assert np.array_equal(ranks[r]["root%d_staged" % root].reshape(held, F, B), full[first:first + held]), (root, r)
    # dedispersion of the gathered band on rank 0 (bf_dedisperse_band_device / bf_dedisperse_dm_band_device): ascending f over
    # ALL channels = the bits a single GPU holding the whole band produces = the oracle's
    assert np.array_equal(ranks[0]["band_ded0"], orc.dedisperse(g, want[0]))
    n_t_out = n_rows - int(delays.max())
    assert np.array_equal(ranks[0]["band_dm"], orc.dedisperse_dm(full, delays, n_t_out))


def test_gather_detected_8_ranks_at_the_true_config4_per_rank_shape(orc, fake_rccl, tmp_path):
    """VERDICT r02 missing item 5: BASELINE configs[3] at the size one rank really runs -- 32 of 256 channels x 256 beams x
    N_TIME 512 (n_ipo 32), 2 gemm-units, the reference's steering fan -- on 8 rank processes; every rank's kernel output and
    the gathered band, in both layouts and all four receiver modes, against the oracle's WHOLE-BAND result, bit for bit."""
    world = 8
    env = dict(os.environ, DSABF_RCCL_LIB=fake_rccl, FAKERCCL_MAILBOX_MB="4", GATHER_SHAPE="c4")
    delays = np.zeros((2, 256), np.int32)
    delays[1] = np.sort(np.random.default_rng(6).integers(0, 4, size=256))[::-1]
    np.save(tmp_path / "delays.npy", delays)
    procs = [subprocess.Popen([sys.executable, os.path.join(SUPPORT, "gather_worker.py"), str(r), str(world), str(tmp_path)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = [p.communicate(timeout=900)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    prob = np.load(tmp_path / "problem.npz")
    w, packed = prob["w"], prob["packed"]
    assert w.shape == (256, 64, 256, 2) and packed.shape == (2, 256, 512, 64)
    F, B, fl = 256, 256, 32
    g = orc.Geom(n_beams=B, n_ant=64, n_freq=F, n_avg=16, n_out_per_gemm=16)
    want = orc.beamform(g, w, packed)                               # [unit][o][256][256]: the whole band
    n_rows = want.shape[0] * want.shape[1]
    full = want.reshape(n_rows, F, B)
    ranks = [np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world)]
    for r in range(world):
        assert np.array_equal(ranks[r]["local"].reshape(n_rows, fl, B), full[:, r * fl:(r + 1) * fl]), r
    shards = np.stack([full[:, r * fl:(r + 1) * fl] for r in range(world)])
    for root in (0, world - 1, -1, -2):
        receivers = [root] if root >= 0 else list(range(world))
        for r in receivers:
            held = n_rows // world if root == -2 else n_rows
            first = r * held if root == -2 else 0
            assert np.array_equal(ranks[r]["root%d_layout0" % root].reshape(held, F, B), full[first:first + held]), (root, r)
            assert np.array_equal(ranks[r]["root%d_layout1" % root].reshape(world, held, fl, B), shards[:, first:first + held]), (root, r)
            assert np.array_equal(ranks[r]["root%d_staged" % root].reshape(held, F, B), full[first:first + held]), (root, r)
    assert np.array_equal(ranks[0]["band_ded0"], orc.dedisperse(g, want[0]))
    assert np.array_equal(ranks[0]["band_dm"], orc.dedisperse_dm(full, delays, n_rows - int(delays.max())))


@pytest.mark.sweep_cap(0)   # DSABF_LONG_TESTS=1 only: the budgeted run keeps `beam -R 2` through test_gpu_round5::test_beam_cli_dm_stage_… (staged
def test_beam_sharded_over_two_ranks_gathers_the_whole_band(orc, fake_rccl, tmp_path):   # transport, -w checked) and the sharded-loop walk (in place)
    """`beam -j 28 -R 2 -r i -I id` (25 burn-in reads + 3 analysed blocks): two shard processes, the detected powers of both gathered to shard 0 after every
    block (bf_gather_detected on the block's compute queue inside run_observation), shard 0 alone writes -w: the file
    holds [gemm][o][256 freq][beam] = shard 0's channels 0..127 next to shard 1's 128..255, bit for bit the oracle's."""
    from dsabeamformer_amd import build, host

    import dsabeamformer_amd as bfm

    env = dict(os.environ, DSABF_RCCL_LIB=fake_rccl)
    out = tmp_path / "band.bin"
    cmd = lambda r: [build.BEAM, "-j", "28", "-R", "2", "-r", str(r), "-D", "0", "-I", str(tmp_path / "id")] + (["-w", str(out)] if r == 0 else [])  # noqa: E731
    procs = [subprocess.Popen(cmd(r), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in (0, 1)]
    outs = [p.communicate(timeout=900)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    assert "Shard 0 of 2: channels 0 .. 127" in outs[0] and "Shard 1 of 2: channels 128 .. 255" in outs[1]
    assert "Wrote 96 gemm-units" in outs[0]
    cfg = bfm.production_config(n_freq=128)                     # one shard's geometry
    n_time = cfg.n_out_per_gemm * cfg.n_pol * cfg.n_avg
    # both shards read the same junk bytes (same seed, same local geometry); their weights are their own channels
    ring = host.junk_bytes(cfg.n_ant * cfg.n_freq * n_time * cfg.n_gemms_per_block, 4, 0xD5A, cfg).reshape(
        4, cfg.n_gemms_per_block, cfg.n_freq, n_time, cfg.n_ant)
    pos, dirs = host.default_positions(64), host.default_directions(256)
    raw = np.fromfile(out, np.float32, offset=4096).reshape(3 * 32, cfg.n_out_per_gemm, 256, 256)
    g = orc.Geom(n_beams=256, n_ant=64, n_freq=128, n_avg=16, n_out_per_gemm=8)
    for gemm in (0, 31, 40, 95):
        blk, ts = divmod(gemm, 32)
        unit = ring[(25 + blk) % 4, ts][None]               # the first 25 blocks of the source went to the burn-in reads
        for r in (0, 1):
            w = host.make_weights(pos, dirs, 128, chan0=128 * r, gpu=0)
            want = orc.beamform(g, w, unit)[0]                  # [o][128][256]
            assert np.array_equal(raw[gemm][:, 128 * r:128 * (r + 1)], want), (gemm, r)


@pytest.mark.parametrize("gather,n,wl", sweep([("alltoall", 2, "c3"), ("root", 2, "c3"), ("alltoall", 8, "c3"), ("alltoall", 8, "c5")],
                                               [("alltoall", 8, "c3"), ("alltoall", 8, "c5")]))
def test_bench_with_two_ranks_on_one_gpu(fake_rccl, gather, n, wl):
    """bench.py as the driver launches it for N = 2 (torch.distributed.run, one process per rank) -- with both ranks on
    GPU 0, gloo for the barrier / max-over-ranks / id broadcast and the loopback stand-in under bf_gather_detected: the
    N > 1 control flow (sharded weights and inputs, double-buffered gather on the side stream, every gather mode side by
    side) runs end to end and rank 0 prints one well-formed line.  The numbers mean nothing (two ranks on one GPU).
    wl = c5: BASELINE configs[4] "on 8 MI355X" -- 100 antennas, 512 beams, 1024 channels = 128 per rank, 256-KiB rows -- as the
    driver would launch it (the committed shape of that line: profiles/r06_bench_c5_n8_loopback.json, --units 16)."""
    import json

    F, B = (1024, 512) if wl == "c5" else (256, 256)

    # (n = 8: the driver's largest launch, 32 channels per rank; 64 rings of 4 MiB keep the shared memory small)
    env = dict(os.environ, DSABF_RCCL_LIB=fake_rccl, DSABF_BENCH_ONE_GPU="1", FAKERCCL_MAILBOX_MB="64" if n == 2 else "4")
    port = str(29700 + os.getpid() % 200)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
                        "127.0.0.1", "--master-port", port, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "3",
                        "--warmup", "1", "--units", "2" if wl == "c5" else "4" if n == 2 else "8", "--workload", wl, "--gather", gather,
                        "--dist-backend", "gloo", "--min-warm-seconds", "0.1", "--no-cpu-baseline", "--full"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                   # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == n and d["config"]["freq_per_gpu"] == F // n and d["scaling"] == "strong"
    assert ("100 ant" in d["config"]["workload"]) == (wl == "c5")
    assert d["config"]["gather"].startswith(gather) and "C-ABI" in d["config"]["gather"] and "gather_note" not in d["config"]
    # what the LIBRARY says about the communicator (bf_comm_info): as many ranks as the launcher started, and which file
    assert d["rccl"]["ranks"] == n and d["rccl"]["lib"].endswith("libfakerccl.so") and d["rccl"]["version"] == 0
    modes = d["gather_modes"]
    for k in ("none", "root_rank_major", "root_freq_major", "root_freq_major_staged", "alltoall_rank_major", "alltoall_freq_major",
              "alltoall_freq_major_staged"):
        assert "error" not in modes[k] and modes[k]["value"] > 0, (k, modes[k])
        assert k == "none" or modes[k]["verified"] is True, (k, modes[k])
    assert modes["%s_rank_major" % gather]["headline"] is True and d["kernel_only"]["value"] == modes["none"]["value"]
    # what the fabric carries per sender and step: one message per (sender, receiver) pair for the rank-major wire and the staged
    # transport, one per (row, sender) for the reference's layout received in place
    n_rows = d["config"]["beam_blocks_per_step"]
    assert modes["alltoall_freq_major"]["messages_sent_per_rank_per_step"] == (n - 1) * (n_rows // n)
    assert modes["alltoall_freq_major_staged"]["messages_sent_per_rank_per_step"] == modes["alltoall_rank_major"]["messages_sent_per_rank_per_step"] == n - 1
    assert modes["root_freq_major"]["messages_sent_per_rank_per_step"] == n_rows and modes["root_freq_major_staged"]["messages_sent_per_rank_per_step"] == 1
    assert modes["alltoall_rank_major"]["bytes_sent_per_rank_per_step"] == n_rows * (F // n) * B * 4 * (n - 1) / n
    # the link model beside it: alltoall loads every link with 1 / n of a rank's powers per direction, root the root's with all of them
    shard = n_rows * (F // n) * B * 4
    lm_a, lm_r = modes["alltoall_rank_major"]["link_model"], modes["root_rank_major"]["link_model"]
    assert lm_a["bytes_on_the_busiest_link_per_step"] == shard / n and lm_r["bytes_on_the_busiest_link_per_step"] == shard
    assert abs(lm_a["ms_at_75_gbs"] - shard / n / 75e9 * 1e3) < 1e-9 and lm_a["measured_gbs_per_link"] > 0 and "link_model" not in modes["none"]


def test_bench_launches_its_own_ranks_when_called_plainly(fake_rccl):
    """`python bench.py --gpus 2` with NO launcher around it (the shape of the driver's N = 1 command):
    bench.py starts torch.distributed.run itself as a child before anything touches the GPU, rank 0's line is the command's
    one line, the exit code is the launcher's.  The line carries the same keys as the N = 1 line: roofline (live HIP-event
    kernel time), cpu_baseline (bounded sample, rank 0's host cores), the library's own rank count, every gather mode."""
    import json

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env.update(DSABF_RCCL_LIB=fake_rccl, DSABF_BENCH_ONE_GPU="1", FAKERCCL_MAILBOX_MB="64")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--units", "4",
                        "--dist-backend", "gloo", "--min-warm-seconds", "0.1", "--cpu-seconds", "1", "--full"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "without a launcher: starting -m torch.distributed.run" in r.stderr
    # stdout is the JSON line and nothing else: what the ranks' native libraries print there (gloo's "[Gloo] Rank 0 is connected to
    # 1 peer ranks", one per rank) goes to stderr (bench.claim_stdout) -- a driver that parses the command's stdout sees one line
    assert r.stdout.count("\n") == 1 and r.stdout.startswith("{"), r.stdout[:600]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["config"]["freq_per_gpu"] == 128
    assert d["rccl"]["ranks"] == 2
    roof = d["roofline"]
    assert roof["bound"] == "mfma" and roof["kernel_ms_avg"] > 0 and 0 < roof["frac"] < 1
    # the per-rank kernel works on half the band: half the algorithmic ops of the whole-band beam-blocks of one step
    assert roof["algorithmic_ops_per_launch"] == 8 * 256 * 64 * 32 * 256 * (4 * 16) // 2
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["unit"] == "beam-blocks/s" and cb["cores"] >= 1
    assert all("error" not in v for k, v in d["gather_modes"].items() if k != "note")
    # every mode is verified after it is timed (checksums of the senders' rows against what the receivers hold), both transports
    # of the freq-major layout included
    modes = {k: v for k, v in d["gather_modes"].items() if k not in ("note", "none")}
    assert set(modes) == {"root_rank_major", "root_freq_major", "root_freq_major_staged", "alltoall_rank_major",
                          "alltoall_freq_major", "alltoall_freq_major_staged"}
    assert all(v["verified"] is True and v["value"] > 0 for v in modes.values()), modes
    assert d["value"] > 0 and "gather_error" not in d and "gloo" in d["config"]["control_plane"]


def _plain_bench(env, *extra, timeout=600):
    env = {k: v for k, v in env.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--units", "4",
                           "--min-warm-seconds", "0.1", "--no-cpu-baseline", *extra], capture_output=True, text=True, timeout=timeout, env=env)


def test_bench_with_a_send_that_never_returns_still_prints_the_kernel_only_record(fake_rccl):
    """a fabric on which the first ncclSend never comes back (the stand-in sleeps forever in it).  The
    kernel-only region was measured before any communicator existed, so the line carries gather_modes.none; the stage that hung
    is named in gather_error; value is null; the command ends NON-ZERO -- in seconds (6 s here; the bound below leaves room for a
    cold, slow box), not at the driver's 1800 s limit."""
    import json
    import time

    env = dict(os.environ, DSABF_RCCL_LIB=fake_rccl, DSABF_BENCH_ONE_GPU="1", FAKERCCL_MAILBOX_MB="64", FAKERCCL_HANG_SEND="1")
    t0 = time.time()
    r = _plain_bench(env, "--gather-timeout", "3")
    took = time.time() - t0
    assert r.returncode != 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, (r.stdout + r.stderr)[-3000:]
    d = json.loads(lines[0])
    assert d["value"] is None and d["n_gpus"] == 2
    assert d["gather_modes"]["none"]["value"] > 0 and d["kernel_only"]["value"] > 0 and 0 < d["kernel_only"]["roofline_frac"] < 1
    assert "alltoall_rank_major" in d["gather_error"] and "did not finish" in d["gather_error"] and d["rank"] == 0
    assert d["stage"].startswith("gather 'alltoall_rank_major'")
    assert d["rccl"]["lib"].endswith("libfakerccl.so")            # the diagnostic names the library that never answered
    assert d["roofline"]["kernel_ms_avg"] > 0                     # the kernel-only region's own roofline record is in the line
    assert took < 150, took


def test_bench_catches_a_gather_that_delivers_wrong_bits(fake_rccl):
    """every gather mode is verified after it is timed (per-row position-weighted checksums, published by
    the senders on the control plane, recomputed by the receivers on what they hold).  A stand-in that flips ONE bit of one
    received message: gather_modes[headline].verified is false, value is null, the command ends non-zero."""
    import json

    env = dict(os.environ, DSABF_RCCL_LIB=fake_rccl, DSABF_BENCH_ONE_GPU="1", FAKERCCL_MAILBOX_MB="64", FAKERCCL_CORRUPT="1")
    r = _plain_bench(env)
    assert r.returncode != 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, (r.stdout + r.stderr)[-3000:]
    d = json.loads(lines[0])
    assert d["gather_modes"]["alltoall_rank_major"]["verified"] is False and d["gather_modes"]["alltoall_rank_major"]["headline"] is True
    assert d["value"] is None and d["unverified_value"] > 0 and "other bits" in d["gather_error"]
    assert d["gather_modes"]["none"]["value"] > 0
    # (the same command on an honest stand-in verifies every mode: test_bench_launches_its_own_ranks_when_called_plainly)


def test_plain_multi_gpu_request_on_this_one_gpu_box_is_refused_without_starting_anything():
    """the parent counts GPUs from sysfs (no HIP, no torch): on a 1-GPU box `bench.py --gpus 2` says so,
    ends non-zero and starts no child.  The sysfs count agrees with what the HIP runtime reports (asked in a child process)."""
    import bench

    n_hip = int(subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True,
                               text=True, timeout=300).stdout.strip())
    assert bench.count_gpus() == n_hip >= 1
    if n_hip >= 2:
        pytest.skip("this box has %d GPUs" % n_hip)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DSABF_BENCH_ONE_GPU")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and "this node shows 1 GPU(s)" in r.stderr and "starting" not in r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]       # refused as a line (value null), both counts in it: the
    d = json.loads(lines[0])                                               # sysfs walk and a child's torch.cuda.device_count() agree
    assert len(lines) == 1 and d["value"] is None and d["gpus_seen"] == {"sysfs": 1, "child_device_count": 1}


def test_bench_exits_nonzero_when_the_communicator_cannot_be_created():
    """a scaling line must never come from a second code path.  With an RCCL that cannot be loaded the
    two-rank bench must FAIL (round 2 fell back to a torch.distributed gather and noted it in config.gather_note)."""
    env = dict(os.environ, DSABF_RCCL_LIB="/nonexistent/librccl.so", DSABF_BENCH_ONE_GPU="1")
    port = str(29900 + os.getpid() % 90)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", port, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2",
                        "--warmup", "1", "--units", "4", "--dist-backend", "gloo", "--min-warm-seconds", "0.1",
                        "--no-cpu-baseline"], capture_output=True, text=True, timeout=900, env=env)
    import json

    assert r.returncode != 0
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                   # round 5: the failure is a LINE -- with no headline in it
    d = json.loads(lines[0])
    assert d["value"] is None and "could not be loaded" in d["gather_error"] and d["stage"].startswith("RCCL communicator")
    assert d["gather_modes"]["none"]["value"] > 0 and set(d["gather_modes"]) == {"none"}      # kernel-only: measured before RCCL
    assert "could not be loaded" in d["rccl"]["error"]


@pytest.mark.parametrize("world", sweep([1, 2, 4], [2]))
def test_plain_c_sharded_example(fake_rccl, tmp_path, world):
    """examples/sharded.c -- the multi-GPU half of the C-ABI from plain C99: `world` processes, each a frequency shard of the
    DEBUG geometry, block launch, gather to rank 0 in the reference's [o][f][b] order (loopback stand-in for RCCL p2p when
    world > 1, no RCCL at all for world 1), D2H of the gathered block; rank 0 checks the band it received."""
    exe = str(tmp_path / "sharded")
    pkg = os.path.join(ROOT, "dsabeamformer_amd")
    b = subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c", "-std=c99", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "sharded.c"), "-o", exe, "-L" + pkg, "-ldsabf",
                        "-Wl,-rpath," + pkg], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, DSABF_RCCL_LIB=fake_rccl)
    idf = str(tmp_path / "id")
    seen = []
    for transport in ([], ["staged"]):          # received in place / one message per sender + the device re-layout pass
        if os.path.exists(idf):
            os.remove(idf)
        procs = [subprocess.Popen([exe, str(r), str(world), idf, "0"] + transport, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                 for r in range(world)]
        outs = [p.communicate(timeout=300)[0] for p in procs]
        assert all(p.returncode == 0 for p in procs), "\n".join(outs)
        assert "gathered 32 rows x 256 channels x 256 beams" in outs[0] and all(("rank %d ok" % r) in outs[r] for r in range(world))
        peaks = [l for l in outs[0].splitlines() if "peak beam" in l]
        assert len(peaks) == 1
        seen.append(peaks[0])
    assert seen[0] == seen[1]                   # the same band either way
    (tmp_path / ("peak%d.txt" % world)).write_text(seen[0])


def test_a_shard_whose_setup_fails_stops_every_shard_before_the_first_gather(fake_rccl, tmp_path):
    """one rank of a sharded observation cannot open its sink.  It used to return on its own -- and the others waited
    for it in the gather behind block 0, with no timeout.  Now every shard exchanges a "ready" flag before the loop
    (observation_options::local_setup_ok, dsabf::comm_all_ok): all three processes end, promptly, with an error that says whose
    setup failed, and nobody wrote a detected file."""
    import json

    prob = dict(world=3, n_beams=64, n_freq_local=4, n_avg=16, n_out=2, n_units=4, n_streams=2, n_blocks=3, ring_blocks=2,
                gather_root=-1, staged=False, n_dm=0, split=False, seed=1, gpu=0, env={}, bad_rank=1)
    json.dump(prob, open(tmp_path / "problem.json", "w"))
    env = dict(os.environ, DSABF_RCCL_LIB=fake_rccl, FAKERCCL_MAILBOX_MB="8")
    procs = [subprocess.Popen([sys.executable, os.path.join(SUPPORT, "shard_loop_worker.py"), str(r), str(tmp_path)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(3)]
    try:
        outs = [p.communicate(timeout=120)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode not in (0, None) for p in procs), outs
    assert "this shard's caller reported a failed setup" in outs[1], outs[1]
    assert "another shard of this run failed its setup" in outs[0] and "another shard of this run failed its setup" in outs[2], outs
    assert not any(os.path.getsize(tmp_path / f) > 4096 for f in os.listdir(tmp_path) if f.startswith("det."))   # (a header at most)


# (soak: DSABF_LONG_TESTS=1 DSABF_SHARD_SEEDS=16:200 walks other seeds)
@pytest.mark.parametrize("seed", sweep(range(*(int(v) for v in os.environ.get("DSABF_SHARD_SEEDS", "0:16").split(":"))), [6]))
def test_sharded_observation_loop_under_random_shapes(orc, fake_rccl, tmp_path, seed):
    """dsabf::run_observation with a communicator, every shard its own process (bfh_run_observation_junk_sharded): random world
    size (2 .. 4), shard geometry, block size, queue count, sub-block launches, ring, transport (in place / staged), receiver
    (one root, the last rank, every rank) and DM stage (none / on the rank(s) that hold the band / split by trials).  Every
    rank that holds the band wrote the oracle's [gemm][o][world * f][b] -- every shard's channels from ITS weights -- and the
    DM files, joined along the trials, are the oracle's [dm][t][b] over the whole observation."""
    import json

    from dsabeamformer_amd import host

    rng = np.random.default_rng(7100 + seed)
    world = int(rng.integers(2, 5))
    n_u = int(rng.choice([4, 8]))
    n_st = int(rng.choice([s for s in (1, 2, 4) if s <= n_u]))
    fl, n_out, n_avg, B = int(rng.choice([4, 8])), int(rng.choice([2, 4])), int(rng.choice([16, 8])), int(rng.choice([64, 128]))
    n_blocks, ring_blocks = int(rng.integers(3, 7)), int(rng.integers(2, 5))
    gather_root = int(rng.choice([0, world - 1, -1]))
    dm_kind = ["none", "holders", "split"][int(rng.integers(3))]
    if dm_kind == "split":
        gather_root = -1
    T, F = n_blocks * n_u * n_out, fl * world
    n_dm = 0 if dm_kind == "none" else int(rng.integers(1, 14))         # fewer trials than ranks happens: a rank with no share
    delays = None
    if n_dm:
        d_max = int(rng.integers(0, max(1, min(T - 2, 2 * n_u * n_out))))
        delays = np.ascontiguousarray((np.arange(n_dm)[:, None] * np.linspace(d_max / max(n_dm - 1, 1), 0.0, F)[None, :]).astype(np.int32))
        np.save(tmp_path / "delays.npy", delays)
    env_in = {}
    if rng.integers(2):
        env_in["DSABF_UNITS_PER_LAUNCH"] = int(rng.choice([1, 2, n_u // 2]))
    prob = dict(world=world, n_beams=B, n_freq_local=fl, n_avg=n_avg, n_out=n_out, n_units=n_u, n_streams=n_st, n_blocks=n_blocks,
                ring_blocks=ring_blocks, gather_root=gather_root, staged=bool(rng.integers(2)), n_dm=n_dm, split=dm_kind == "split",
                seed=3000 + seed, gpu=int(rng.integers(0, 3)), env=env_in)
    json.dump(prob, open(tmp_path / "problem.json", "w"))
    env = dict(os.environ, DSABF_RCCL_LIB=fake_rccl, FAKERCCL_MAILBOX_MB="8")
    procs = [subprocess.Popen([sys.executable, os.path.join(SUPPORT, "shard_loop_worker.py"), str(r), str(tmp_path)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), (prob, "\n".join(outs))
    ranks = [np.load(tmp_path / ("rank%d.npz" % r)) for r in range(world)]
    g = orc.Geom(n_beams=B, n_ant=64, n_freq=fl, n_avg=n_avg, n_out_per_gemm=n_out)
    pos, dirs = host.default_positions(64), host.default_directions(B)
    band = []
    for r in range(world):     # every shard read the same junk bytes with its local geometry; its weights are its own channels
        w = host.make_weights(pos, dirs, fl, chan0=fl * r, gpu=prob["gpu"])
        ring = ranks[r]["ring"]
        band.append(np.concatenate([orc.beamform(g, w, ring[b % ring_blocks]).reshape(n_u * n_out, fl, B) for b in range(n_blocks)]))
    series = np.concatenate(band, axis=1)                              # [T][F][B]
    holders = list(range(world)) if gather_root < 0 else [gather_root]
    for r in range(world):
        assert os.path.exists(tmp_path / ("det.%d" % r)) == (r in holders), (prob, r)
    for r in holders:
        hdr, data = host.read_detected_file(str(tmp_path / ("det.%d" % r)))
        assert int(hdr["N_FREQUENCIES"]) == F, (prob, r)
        assert np.array_equal(data.reshape(series.shape), series), (prob, r)
    if n_dm:
        D = int(delays.max())
        want = orc.dedisperse_dm(series, delays, T - D)
        for r in holders:
            first, count = host.dm_trial_share(n_dm, world, r) if prob["split"] else (0, n_dm)
            path = tmp_path / ("dm.%d" % r)
            if count == 0:
                assert not os.path.exists(path) and int(ranks[r]["dm_times"]) == 0, (prob, r)
                continue
            d_r = int(delays[first:first + count].max())               # a rank's window is its OWN trials' largest delay
            hdr, got, chunks = host.read_dm_file(str(path))
            assert int(hdr["DM_FIRST_TRIAL"]) == first and int(hdr["N_DM"]) == count and int(hdr["MAX_DELAY"]) == d_r, (prob, r)
            assert int(ranks[r]["dm_times"]) == T - d_r == got.shape[1], (prob, r)
            assert np.array_equal(got[:, :T - D], want[first:first + count]), (prob, r)
            if d_r < D:       # the rank's shorter window gives it more output times than the whole ladder's: check those too
                assert np.array_equal(got, orc.dedisperse_dm(series, delays[first:first + count], T - d_r)), (prob, r)
