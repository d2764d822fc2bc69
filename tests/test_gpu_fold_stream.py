"""GPU tests (-m gpu) of the streamed antenna-fold kernels (fused16_fold_stream_kernel, csrc/bf_fused16.hpp): the fold kernel of
gemm-units that are whole chunk spans (T % 128 == 0; T % 256 == 0 for the 64-sample window).  Its chunk addressing is scalar state
that steps by a constant, its prefetch is unconditional and clamped to the workgroup's last chunk, and nothing in it tests a sample
against the launch's end -- so the shapes here are the smallest at which each of those can go wrong.  Every case is held to the CPU
oracle bit for bit the way tests/test_gpu_fold.py holds the fold kernel (the fast reading to its stated tolerance as well), to the
same handle on the kernel it runs after set_switch("fold", 0) byte for byte, and to the NaN guard behind the last output."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANONICAL, FAST, CONTRACTED = 0, 1, 2
STREAM, PER_ROW = "fused16_fold_stream_kernel", "fused16_fold_kernel"


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


def config(bfmod, g, mode=CANONICAL):
    return bfmod.production_config(n_beams=g.n_beams, n_ant=g.n_ant, n_freq=g.n_freq, n_pol=g.n_pol, n_avg=g.n_avg,
                                   n_out_per_gemm=g.n_out_per_gemm, n_gemms_per_block=1, n_blocks_on_gpu=1, n_streams=1, detect_mode=mode)


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


def check(orc, g, w, packed, got, mode):
    if mode == FAST:
        want = orc.beamform_fast(g, w, packed)
        exact = orc.beamform_exact(g, w, packed)
        ok = exact > 0
        assert np.abs(got[ok] / exact[ok] - 1).max() <= (g.n_ipo + 1) * 2.0 ** -23, "fast detect outside its stated tolerance"
    else:
        with orc.detect_contract(orc.CONTRACT_NVCC if mode == CONTRACTED else orc.CONTRACT_NONE):
            want = orc.beamform(g, w, packed)
    assert np.array_equal(got, want), "differs from the oracle in %d of %d values" % ((got != want).sum(), want.size)


# (n_freq, n_beams, n_avg, n_out_per_gemm, gemm-units, detect reading, tsplit): T = 2 n_avg n_out samples per gemm-unit, n_ipo = 2 n_avg;
# tsplit 1 = one workgroup per frequency and beam group walks every chunk of the launch (0: the library's own split).
#   n_freq 3 / 8: the two block maps; n_beams 256: four waves, 16-byte stores; 64: one wave with beams, three that only stage (the
#   loop of their own); 80: scalar stores and a part-filled tile.
SHAPES = [
    # workgroups of 1, 2, 3, 4 chunks (n_ipo 32, T = 128): the prologue's two requests, the clamped ones, the extra image of the last chunk
    (3, 256, 16, 4, 1, CANONICAL, 1), (8, 64, 16, 4, 2, CANONICAL, 1), (3, 80, 16, 4, 3, CANONICAL, 1), (8, 256, 16, 4, 4, CANONICAL, 1),
    # T = 256 x 3 units: six chunks in one workgroup; tsplit 4: chunk ranges of 1, 2, 1, 2 that start inside a gemm-unit
    (3, 256, 16, 8, 3, CANONICAL, 1), (8, 80, 16, 8, 3, CANONICAL, 4), (3, 64, 16, 8, 3, CANONICAL, 4),
    # the scalar step across gemm-units: T = 128 x 5 (every chunk a new unit); T = 384 x 3 (every third chunk, T no power of two: the
    # division in the workgroup's first address; tsplit 2 starts the second workgroup at chunk 4 = sample 128 of unit 1)
    (3, 64, 16, 4, 5, CANONICAL, 1), (8, 256, 16, 4, 5, CANONICAL, 0),
    (3, 256, 16, 12, 3, CANONICAL, 1), (8, 80, 16, 12, 3, CONTRACTED, 2), (3, 64, 16, 12, 3, FAST, 0),
    # n_ipo 16, T = 128 and 256: two outputs parked per chunk; 1 and 3 units
    (3, 256, 8, 8, 1, CANONICAL, 1), (8, 80, 8, 8, 3, FAST, 1), (3, 64, 8, 16, 1, CONTRACTED, 1), (8, 256, 8, 16, 3, CANONICAL, 1),
    # n_ipo 64, T = 256 and 512: spans of 256 samples, two chunks per group; 1 and 3 units
    (3, 256, 32, 4, 1, CANONICAL, 1), (8, 64, 32, 4, 3, CANONICAL, 1), (3, 80, 32, 8, 1, CONTRACTED, 1), (8, 256, 32, 8, 3, FAST, 1),
]


@pytest.mark.sweep_cap(len(SHAPES))
@pytest.mark.parametrize("shape", SHAPES, ids=["f%d-b%d-avg%d-out%d-u%d-m%d-ts%d" % s for s in SHAPES])
def test_whole_span_units_run_the_streamed_kernel_bit_exact(torch, bfmod, orc, shape):
    n_freq, n_beams, n_avg, n_out, n_units, mode, tsplit = shape
    g = orc.Geom(n_beams=n_beams, n_ant=64, n_freq=n_freq, n_avg=n_avg, n_out_per_gemm=n_out)
    assert g.n_time % (256 if g.n_ipo == 64 else 128) == 0
    rng = np.random.default_rng(8000 + sum((i + 1) * v for i, v in enumerate(shape)))
    w = antenna_symmetric(rng.integers(-127, 128, size=(g.n_freq, g.n_ant, g.n_beams, 2), dtype=np.int8))   # beams: no symmetry
    packed = rng.integers(0, 256, size=(n_units, g.n_freq, g.n_time, g.n_ant), dtype=np.uint8)
    with bfmod.Beamformer(config(bfmod, g, mode)) as bf:
        bf.set_switch("tsplit", tsplit)
        bf.set_weights(w)
        info = bf.kernel_info(n_units)
        assert "FOLD" in info["kernel"] and "PAIRED" not in info["kernel"], info
        assert bf.variant_key() == "fused16_fold_kernel<%d, %d>" % (g.n_ipo, mode)          # the label names the family
        assert info["launch"] == STREAM, info
        if tsplit:
            bgroups = (n_beams + 255) // 256
            assert info["grid"] == n_freq * bgroups * tsplit, info
        got = run(torch, bf, g, packed)
        bf.set_switch("fold", 0)                           # the same handle on the general kernel
        bf.set_weights(w)
        info = bf.kernel_info(n_units)
        assert "FOLD" not in info["kernel"] and info["launch"] == "fused16_kernel", info
        other = run(torch, bf, g, packed)
    assert got.tobytes() == other.tobytes()
    check(orc, g, w, packed, got, mode)


def test_selection_by_the_gemm_unit_and_the_switches(torch, bfmod, orc, monkeypatch):
    """T = 96 keeps fused16_fold_kernel and its per-row addressing, T = 128 runs the streamed kernel; n_ipo 64 needs T % 256 == 0;
    set_switch("fold", 0) and DSABF_PAIRED select what they selected before."""
    for n_avg, n_out, launch in ((16, 3, PER_ROW), (16, 4, STREAM), (32, 6, PER_ROW), (32, 4, STREAM), (8, 4, PER_ROW), (8, 8, STREAM)):
        g = orc.Geom(n_beams=64, n_ant=64, n_freq=3, n_avg=n_avg, n_out_per_gemm=n_out)
        w = orc.make_weights(g, orc.default_positions(g.n_ant), orc.default_directions(g.n_beams), 0)     # both symmetries
        packed = np.random.default_rng(8100 + n_avg + n_out).integers(0, 256, size=(2, g.n_freq, g.n_time, g.n_ant), dtype=np.uint8)
        with bfmod.Beamformer(config(bfmod, g)) as bf:
            bf.set_weights(w)
            info = bf.kernel_info(2)
            assert "PAIRED,FOLD" in info["kernel"] and info["launch"] == launch, (g.n_time, info)
            assert bf.variant_key() == "fused16_fold_kernel<%d, 0>" % g.n_ipo
            assert bf.counter("fold_stream") == (launch == STREAM)
            got = run(torch, bf, g, packed)
            check(orc, g, w, packed, got, CANONICAL)
            if (n_avg, n_out) != (16, 4):
                continue
            bf.set_switch("fold", 0)
            bf.set_weights(w)
            info = bf.kernel_info(2)
            assert "PAIRED" in info["kernel"] and "FOLD" not in info["kernel"] and info["launch"] == "fused16_kernel", info
            assert bf.variant_key() == "fused16_kernel<-1, 32, false, 0, true, 4, 4>" and bf.counter("fold_stream") == 0
            assert run(torch, bf, g, packed).tobytes() == got.tobytes()
            bf.set_switch("fold", 1)
            for value, paired in (("pair", True), ("0", False)):
                monkeypatch.setenv("DSABF_PAIRED", value)
                bf.set_weights(w)
                info = bf.kernel_info(2)
                assert "FOLD" not in info["kernel"] and ("PAIRED" in info["kernel"]) == paired and info["launch"] == "fused16_kernel", info
                assert run(torch, bf, g, packed).tobytes() == got.tobytes()
            monkeypatch.delenv("DSABF_PAIRED")
            bf.set_weights(w)
            assert bf.kernel_info(2)["launch"] == STREAM
