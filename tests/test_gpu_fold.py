"""GPU tests (-m gpu) of the antenna-fold kernel (fused16_fold_kernel, csrc/bf_fused16.hpp): 64 antennas whose weights satisfy
W[f][63-a][b] == conj(W[f][a][b]) -- any array that is point-symmetric about its phase centre -- run one K = 64 MFMA per output row
on the sums and differences of the 32 mirror pairs.  The integers it accumulates are the integers of the other kernels, so every
detect reading is held to the oracle bit for bit (np.array_equal), the fast reading the way tests/test_gpu_census.py holds it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANONICAL, FAST, CONTRACTED = 0, 1, 2


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


# (n_freq, n_beams, n_avg, n_out_per_gemm, gemm-units, detect reading)
#   n_freq 3 / 8: the two block maps (decode_block); n_beams 256: four waves, interleaved 16-byte stores; 64: one wave with beams,
#   three that only stage; 80: tile-by-tile scalar stores and a partly filled last tile; T = 256 x 3 units: scalar chunk addressing,
#   6 chunks; T = 96 x 5 units: per-row addressing across gemm-units and a ragged tail; n_ipo 16 and 64: the other two windows.
SHAPES = [
    (3, 256, 16, 8, 3, CANONICAL), (3, 256, 16, 8, 3, CONTRACTED), (3, 256, 16, 8, 3, FAST),
    (8, 256, 16, 3, 5, CANONICAL),
    (3, 64, 16, 8, 3, CANONICAL), (8, 64, 16, 3, 5, CANONICAL),
    (8, 80, 16, 8, 3, CANONICAL), (3, 80, 16, 3, 5, CANONICAL),
    (3, 256, 8, 16, 3, CANONICAL), (3, 80, 8, 6, 5, CONTRACTED),
    (8, 256, 32, 4, 5, CANONICAL), (3, 80, 32, 3, 3, FAST),
]


@pytest.mark.sweep_cap(len(SHAPES))
@pytest.mark.parametrize("shape", SHAPES, ids=["f%d-b%d-avg%d-out%d-u%d-m%d" % s for s in SHAPES])
def test_antenna_symmetric_weights_run_the_fold_kernel_bit_exact(torch, bfmod, orc, shape):
    n_freq, n_beams, n_avg, n_out, n_units, mode = shape
    g = orc.Geom(n_beams=n_beams, n_ant=64, n_freq=n_freq, n_avg=n_avg, n_out_per_gemm=n_out)
    rng = np.random.default_rng(7000 + sum((i + 1) * v for i, v in enumerate(shape)))
    w = antenna_symmetric(rng.integers(-127, 128, size=(g.n_freq, g.n_ant, g.n_beams, 2), dtype=np.int8))   # beams: no symmetry
    packed = rng.integers(0, 256, size=(n_units, g.n_freq, g.n_time, g.n_ant), dtype=np.uint8)
    with bfmod.Beamformer(config(bfmod, g, mode)) as bf:
        bf.set_weights(w)
        name = bf.kernel_info(n_units)["kernel"]
        assert "FOLD" in name and "PAIRED" not in name, name
        assert bf.variant_key() == "fused16_fold_kernel<%d, %d>" % (g.n_ipo, mode)
        got = run(torch, bf, g, packed)
    check(orc, g, w, packed, got, mode)


def test_extreme_sums_and_differences_against_the_largest_weights(torch, bfmod, orc):
    """Packed bytes 0x88 / 0x77 on both antennas of every mirror pair (S = -16 and +14) and 0x87 against 0x78 (D = -+15 in the real,
    +-15 in the imaginary part), against weights of +-127 in every sign pattern: the ends of the staged int8 range and the largest sums."""
    g = orc.Geom(n_beams=64, n_ant=64, n_freq=3, n_avg=16, n_out_per_gemm=8)
    rng = np.random.default_rng(7100)
    w = np.empty((g.n_freq, g.n_ant, g.n_beams, 2), np.int8)
    b = np.arange(g.n_beams)
    w[..., 0] = np.where(b & 1, -127, 127)[None, None, :]
    w[..., 1] = np.where(b & 2, -127, 127)[None, None, :]
    w[:, ::3, 32:, :] *= -1                                # ... and, for half the beams, signs that alternate along the array
    w = antenna_symmetric(w)
    packed = rng.integers(0, 256, size=(3, g.n_freq, g.n_time, g.n_ant), dtype=np.uint8)
    for t, (lo, hi) in enumerate(((0x88, 0x88), (0x77, 0x77), (0x87, 0x78), (0x78, 0x87), (0x88, 0x77), (0x77, 0x88))):
        for t0 in (0, 37, 128 + 64, 255 - 6):              # first rows, mid-chunk, second chunk, the unit's last rows
            packed[:, :, t0 + t, :32] = lo
            packed[:, :, t0 + t, 32:] = hi
    packed[2, 1] = 0x88                                    # a whole gemm-unit of (-8, -8)
    packed[2, 2, :, :32], packed[2, 2, :, 32:] = 0x87, 0x78
    with bfmod.Beamformer(config(bfmod, g)) as bf:
        bf.set_weights(w)
        assert "FOLD" in bf.kernel_info(3)["kernel"]
        got = run(torch, bf, g, packed)
    check(orc, g, w, packed, got, CANONICAL)


def test_default_fan_has_both_symmetries_and_fold_equals_the_pair_kernel(torch, bfmod, orc):
    g = orc.Geom(n_beams=256, n_ant=64, n_freq=8, n_avg=16, n_out_per_gemm=8)
    w = orc.make_weights(g, orc.default_positions(g.n_ant), orc.default_directions(g.n_beams), 0)
    packed = np.random.default_rng(7200).integers(0, 256, size=(3, g.n_freq, g.n_time, g.n_ant), dtype=np.uint8)
    with bfmod.Beamformer(config(bfmod, g)) as bf:
        bf.set_weights(w)
        name = bf.kernel_info(3)["kernel"]
        assert "PAIRED" in name and "FOLD" in name, name
        shape = {k: v for k, v in bf.kernel_info(3).items() if k in ("grid", "block", "lds_bytes")}
        got = run(torch, bf, g, packed)
        bf.set_switch("fold", 0)                           # the same handle on the conjugate-pair kernel
        bf.set_weights(w)
        name = bf.kernel_info(3)["kernel"]
        assert "PAIRED" in name and "FOLD" not in name, name
        assert bf.variant_key() == "fused16_kernel<-1, 32, false, 0, true, 4, 4>"
        assert shape == {k: v for k, v in bf.kernel_info(3).items() if k in shape}     # the pair kernel's launch shape
        pair = run(torch, bf, g, packed)
    assert np.array_equal(got, pair)
    check(orc, g, w, packed, got, CANONICAL)


def test_one_weight_off_by_one_is_not_folded(torch, bfmod, orc):
    g = orc.Geom(n_beams=64, n_ant=64, n_freq=3, n_avg=16, n_out_per_gemm=3)
    rng = np.random.default_rng(7300)
    w0 = antenna_symmetric(rng.integers(-126, 127, size=(g.n_freq, g.n_ant, g.n_beams, 2), dtype=np.int8))
    packed = rng.integers(0, 256, size=(2, g.n_freq, g.n_time, g.n_ant), dtype=np.uint8)
    with bfmod.Beamformer(config(bfmod, g)) as bf:
        for f, a, b, c in ((0, 0, 0, 0), (2, 63, 63, 1), (1, 31, 17, 1), (1, 32, 40, 0)):
            w = w0.copy()
            w[f, a, b, c] += 1
            bf.set_weights(w)
            assert "FOLD" not in bf.kernel_info(2)["kernel"], (f, a, b, c)
            check(orc, g, w, packed, run(torch, bf, g, packed), CANONICAL)
        bf.set_weights(w0)
        assert "FOLD" in bf.kernel_info(2)["kernel"]


@pytest.mark.parametrize("how", ["fold", "paired", "DSABF_PAIRED"])
def test_the_switches_that_remove_the_fold(torch, bfmod, orc, monkeypatch, how):
    """bf_set_switch(h, "fold", 0) rules out the fold kernel alone; "paired" = 0 and DSABF_PAIRED=0 force the general kernel."""
    g = orc.Geom(n_beams=64, n_ant=64, n_freq=3, n_avg=16, n_out_per_gemm=3)
    w = orc.make_weights(g, orc.default_positions(g.n_ant), orc.default_directions(g.n_beams), 0)     # both symmetries
    packed = np.random.default_rng(7400).integers(0, 256, size=(2, g.n_freq, g.n_time, g.n_ant), dtype=np.uint8)
    with bfmod.Beamformer(config(bfmod, g)) as bf:
        bf.set_weights(w)
        assert "PAIRED,FOLD" in bf.kernel_info(2)["kernel"]
        if how == "DSABF_PAIRED":
            monkeypatch.setenv("DSABF_PAIRED", "0")
        else:
            bf.set_switch(how, 0)
        bf.set_weights(w)
        name = bf.kernel_info(2)["kernel"]
        assert "FOLD" not in name and ("PAIRED" in name) == (how == "fold"), name
        check(orc, g, w, packed, run(torch, bf, g, packed), CANONICAL)


def test_a_large_lds_pad_hands_the_handle_back_to_the_pair_kernel(torch, bfmod, orc):
    """The fold kernel's launcher takes the default 48 KiB of dynamic LDS at most: the "lds_pad" measurement switch beyond that runs
    the kernel the weights select otherwise (here the conjugate-pair kernel), at once and at the next bf_set_weights; same bits."""
    g = orc.Geom(n_beams=64, n_ant=64, n_freq=3, n_avg=16, n_out_per_gemm=3)
    w = orc.make_weights(g, orc.default_positions(g.n_ant), orc.default_directions(g.n_beams), 0)
    packed = np.random.default_rng(7500).integers(0, 256, size=(2, g.n_freq, g.n_time, g.n_ant), dtype=np.uint8)
    with bfmod.Beamformer(config(bfmod, g)) as bf:
        bf.set_weights(w)
        bf.set_switch("lds_pad", 8 * 1024)                 # 32 + 8 KiB: still the fold kernel
        assert "PAIRED,FOLD" in bf.kernel_info(2)["kernel"] and bf.kernel_info(2)["lds_bytes"] == 40 * 1024
        check(orc, g, w, packed, run(torch, bf, g, packed), CANONICAL)
        bf.set_switch("lds_pad", 32 * 1024)
        name = bf.kernel_info(2)["kernel"]
        assert "PAIRED" in name and "FOLD" not in name and bf.kernel_info(2)["lds_bytes"] == 64 * 1024, name
        check(orc, g, w, packed, run(torch, bf, g, packed), CANONICAL)
        bf.set_weights(w)
        assert "FOLD" not in bf.kernel_info(2)["kernel"]
        bf.set_switch("lds_pad", 0)
        bf.set_weights(w)
        assert "PAIRED,FOLD" in bf.kernel_info(2)["kernel"]
        check(orc, g, w, packed, run(torch, bf, g, packed), CANONICAL)
