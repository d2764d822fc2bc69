"""GPU tests (-m gpu) of the streamed antenna-fold kernel's staging (fold_stage_pair, csrc/bf_fold_staging.h; docs/LOG_r09.md): the
byte-wise sums and differences of mirror antennas are formed with guard bits and masks instead of the unfolded statement the
non-stream fold kernel keeps, the LDS addresses of the staging stores and fragment reads step between the two buffers as per-lane
registers, and the output rows' base advances by one scalar add per store.  A wrong carry or borrow between the bytes of a dword
shows at the extreme nibbles, a wrong buffer or row step at workgroups of more than one chunk, so every window and every detect
reading runs

  * inputs of all-0x00, all-0x88 (the most negative nibble in both fields), all-0x77 (the most positive) and seeded random bytes,
  * n_freq 2; 64 beams (one wave with beams, three that only stage) and 256 (four waves); gemm-units of one span and of three
    (T = 128 / 384; 256 / 768 for the 64-sample window); 1 and 3 gemm-units,
  * tsplit values that give workgroups of 1, 2 and 3 chunks (of 1, 2 and 3 two-chunk groups for the 64-sample window, whose
    workgroups hold whole groups),

each bit for bit against the CPU oracle (the fast reading to its stated tolerance as well, as tests/test_gpu_fold_stream.py holds it)
and byte for byte against the same handle on the general kernel after set_switch("fold", 0)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANONICAL, FAST, CONTRACTED = 0, 1, 2
STREAM = "fused16_fold_stream_kernel"
NIPOS, MODES = (16, 32, 64), (CANONICAL, FAST, CONTRACTED)
CASES = [(n, m) for n in NIPOS for m in MODES]

# (n_beams, spans per gemm-unit, gemm-units, tsplit) -> chunks (n_ipo 64: groups) per workgroup.  Every pairing of the two beam
# counts with the two unit lengths, both unit counts, workgroups of 1, 2 and 3.
LAYOUTS = [
    (256, 1, 1, 1),   # 1: the prologue's two requests both clamped
    (256, 1, 3, 3),   # 1, 1, 1: every workgroup starts in another gemm-unit
    (64, 3, 1, 2),    # 1 and 2: the second workgroup starts inside the gemm-unit
    (64, 1, 3, 1),    # 3: a new gemm-unit at every chunk, both buffers written twice
    (256, 3, 3, 3),   # 3, 3, 3
]
FILLS = (0x00, 0x88, 0x77, None)   # None: seeded random bytes


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "these tests need a GPU"
    return t


@pytest.fixture(scope="module")
def bfmod():
    import dsabeamformer_amd as m

    return m


def antenna_symmetric(w):
    """W[:, A-1-a] = conj(W[:, a]): the second half of the antennas mirrors the first."""
    w = w.copy()
    na = w.shape[1]
    w[:, na // 2:, :, 0] = w[:, :na // 2, :, 0][:, ::-1]
    w[:, na // 2:, :, 1] = -w[:, :na // 2, :, 1][:, ::-1]
    return w


def run(torch, bf, g, packed):
    """Detected output [unit][o][f][b] of the handle; the floats behind the last output must stay untouched."""
    n = packed.shape[0] * g.out_per_gemm
    d_in = torch.from_numpy(packed).cuda()
    d_out = torch.full((n + 64,), float("nan"), dtype=torch.float32, device="cuda")
    bf.beamform(d_in, packed.shape[0], d_out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert np.isnan(got[n:]).all(), "wrote behind the last output"
    return got[:n].reshape(packed.shape[0], g.n_out_per_gemm, g.n_freq, g.n_beams)


def check(orc, g, w, packed, got, mode, what):
    if mode == FAST:
        want = orc.beamform_fast(g, w, packed)
        exact = orc.beamform_exact(g, w, packed)
        ok = exact > 0
        if ok.any():
            assert np.abs(got[ok] / exact[ok] - 1).max() <= (g.n_ipo + 1) * 2.0 ** -23, "fast detect outside its stated tolerance: %s" % (what,)
    else:
        with orc.detect_contract(orc.CONTRACT_NVCC if mode == CONTRACTED else orc.CONTRACT_NONE):
            want = orc.beamform(g, w, packed)
    assert np.array_equal(got, want), "%s: differs from the oracle in %d of %d values" % (what, (got != want).sum(), want.size)


@pytest.mark.sweep_cap(len(CASES))
@pytest.mark.parametrize("n_ipo,mode", CASES, ids=["nipo%d-mode%d" % c for c in CASES])
def test_staging_is_bit_exact_at_the_extreme_nibbles_and_every_workgroup_length(torch, bfmod, orc, n_ipo, mode):
    span = 256 if n_ipo == 64 else 128
    for n_beams, spans, n_units, tsplit in LAYOUTS:
        n_out = spans * span // n_ipo
        g = orc.Geom(n_beams=n_beams, n_ant=64, n_freq=2, n_avg=n_ipo // 2, n_out_per_gemm=n_out)
        assert g.n_ipo == n_ipo and g.n_time == spans * span
        rng = np.random.default_rng(9000 + 7 * n_ipo + 3 * mode + n_beams + 11 * spans + 13 * n_units + tsplit)
        w = antenna_symmetric(rng.integers(-127, 128, size=(g.n_freq, g.n_ant, g.n_beams, 2), dtype=np.int8))   # beams: no symmetry
        inputs = []
        for fill in FILLS:
            shape = (n_units, g.n_freq, g.n_time, g.n_ant)
            inputs.append(rng.integers(0, 256, size=shape, dtype=np.uint8) if fill is None else np.full(shape, fill, dtype=np.uint8))
        cfg = bfmod.production_config(n_beams=g.n_beams, n_ant=g.n_ant, n_freq=g.n_freq, n_pol=g.n_pol, n_avg=g.n_avg, n_out_per_gemm=g.n_out_per_gemm,
                                      n_gemms_per_block=1, n_blocks_on_gpu=1, n_streams=1, detect_mode=mode)
        with bfmod.Beamformer(cfg) as bf:
            bf.set_switch("tsplit", tsplit)
            bf.set_weights(w)
            info = bf.kernel_info(n_units)
            assert "FOLD" in info["kernel"] and info["launch"] == STREAM and bf.counter("fold_stream") == 1, info
            assert info["grid"] == g.n_freq * tsplit, info               # one beam group: the split alone multiplies the workgroups
            folded = [run(torch, bf, g, p) for p in inputs]
            bf.set_switch("fold", 0)                                     # the same handle on the general kernel
            bf.set_weights(w)
            info = bf.kernel_info(n_units)
            assert "FOLD" not in info["kernel"] and info["launch"] == "fused16_kernel", info
            general = [run(torch, bf, g, p) for p in inputs]
        for fill, p, got, other in zip(FILLS, inputs, folded, general):
            what = (n_beams, spans, n_units, tsplit, "random" if fill is None else hex(fill))
            assert got.tobytes() == other.tobytes(), "%s: differs from the general kernel" % (what,)
            check(orc, g, w, p, got, mode, what)
