"""The shared-window DM kernel (csrc/bf_dm_wide.hip) path by path: which trial groups it takes, which of its code paths a ladder of
delays reaches, and the inputs of tests/test_gpu_dm_paths.py -- made here so that tests/test_dm_paths_cpu.py can hold every case to
what it claims without a GPU.  numpy only; nothing is drawn at import, every builder seeds its own generator.

The kernel and dedisperse_dm_kernel give the same bits by design, so a bit-exact result says nothing about which of them computed
it.  bf_get_counter "dm_wide_mask" reports what the device decided; wide_fits() below predicts it from the delays alone."""
import numpy as np

# ---- restated from csrc/bf_dm_wide.hip:57-70 and csrc/bf_kernels.h:107-111 ------------------------------------------------------
TRIALS = 32                       # bf_kernels.h: kDwTrials = 2 * kDwWavesPerWg
WAVES = 16                        # bf_kernels.h: kDwWavesPerWg
MAX_GROUPS = 4096                 # bf_kernels.h: kDwMaxGroups
MAX_FREQ = 1024                   # bf_kernels.h: kDwMaxFreq
TB = 16                           # bf_dm_wide.hip: kDwTb, output times per tile
BEAMS = 128                       # kDwBeams = 32 * kDwBpl, kDwBpl = 64 / kDwTb
ROW_BYTES = BEAMS * 4             # kDwRowBytes
ROWS_PER_DMA = 1024 // ROW_BYTES  # kDwRowsPerDma: 2
MAX_ROWS = min(4 * ROWS_PER_DMA * WAVES, 224)   # kDwMaxRows: 128
SLACK_ROWS = 4                    # kDwSlackRows
NBUF = 3                          # kDwNbuf
PIECES = 4                        # kDwPairsPerWave
LDS_BYTES = 160 * 1024 // (16 // WAVES) - 1024   # kDwLdsBytes

PAIR_CLASSES = (0, 1, 2, 3, ">=4", "<0")


def table_bytes(n_freq):
    """dw_table_bytes (csrc/bf_dm_wide.hip:74): the offsets (one byte per trial and channel) and {base, rows} (two ints per
    channel), rounded up to 512."""
    return (n_freq * (TRIALS + 8) + 511) & ~511


def rows_cap(n_freq):
    """dw_rows_cap (csrc/bf_dm_wide.hip:75-80): the window rows one of the three ring buffers holds once the tables and the slack
    are taken out of the LDS."""
    r = ((LDS_BYTES - table_bytes(n_freq) - SLACK_ROWS * ROW_BYTES) // (NBUF * ROW_BYTES)) & ~(ROWS_PER_DMA - 1)
    return min(r, MAX_ROWS)


def groups_of(delays):
    delays = np.asarray(delays)
    return [delays[g0:g0 + TRIALS] for g0 in range(0, delays.shape[0], TRIALS)]


def wide_fits(delays):
    """One bool per group of 32 trials: does dedisperse_dm_wide_kernel take it?  The kernel's fit test (csrc/bf_dm_wide.hip:145: `fits &=
    hi - lo + kDwTb <= rows_cap && lo > -(1 << 30) && hi < (1 << 30)`, every channel, reduced over the workgroup at :152) behind
    dm_wide_supported (csrc/bf_dm_wide.hip:362-365: n_freq <= kDwMaxFreq, 1 .. kDwMaxGroups groups).  The launcher's other gates
    (csrc/bf_kernels.hip:917-919: the switch, alignment, 4 GiB) are not a property of the delays."""
    delays = np.asarray(delays, np.int64)
    n_dm, n_f = delays.shape
    groups = groups_of(delays)
    if n_f > MAX_FREQ or n_dm <= 0 or len(groups) > MAX_GROUPS:
        return np.zeros(len(groups), bool)
    cap = rows_cap(n_f)
    out = []
    for d in groups:
        lo, hi = d.min(axis=0), d.max(axis=0)
        out.append(bool(np.all(hi - lo + TB <= cap) and np.all(lo > -(1 << 30)) and np.all(hi < (1 << 30))))
    return np.array(out, bool)


def mask_of(fits):
    return sum(1 << g for g, f in enumerate(fits) if f and g < 64)


def pieces_per_wave(rows):
    """dma_window (csrc/bf_dm_wide.hip:194-205, 210-212): wave w issues piece j while kDwRowsPerDma * (w + kDwWaves * j) < rows.
    [16] counts for a window of `rows` rows."""
    w = np.arange(WAVES)[:, None]
    j = np.arange(PIECES)[None, :]
    return (ROWS_PER_DMA * (w + WAVES * j) < rows).sum(axis=1)


def census(delays, n_t, n_t_out, n_b):
    """Which paths of the kernel the groups that fit reach:
      pairs       pair-distance classes of PAIR_CLASSES, over the waves whose two trials both exist and all channels: the body the
                  wave runs at that channel (DW_BODY_ALL: delta 0 .. 3 one body each, everything else -- also B before A -- DW_BODY_OWN)
      pieces      LDS-DMA instructions one wave issues for one window, 0 .. 4
      paths       "inside" (tab[f].y bit 16: buffer-addressed) and / or "lane" (per-lane addresses), over tiles and channels
      lane_kinds  why a window is not inside: "before_start", "past_end" (wholly), "straddle_end" (a two-row piece with one row in the
                  series and one past it), "partial_beams"
      mixed_tile  some tile stages some channels on one path and some on the other
      piece_runs  the per-wave piece counts of consecutive channels differ somewhere (what wait_dma_but has to follow)"""
    delays = np.asarray(delays, np.int64)
    fits = wide_fits(delays)
    pairs, pieces, paths, kinds = set(), set(), set(), set()
    mixed = runs = False
    n_y, n_bg = (n_t_out + TB - 1) // TB, (n_b + BEAMS - 1) // BEAMS
    for d, fit in zip(groups_of(delays), fits):
        if not fit:
            continue
        nk = d.shape[0]
        for w in range(nk // 2):                          # waves whose trial B exists (a missing trial repeats the last: never stored)
            for delta in (d[2 * w + 1] - d[2 * w]).tolist():
                pairs.add("<0" if delta < 0 else ">=4" if delta >= 4 else int(delta))
        lo, hi = d.min(axis=0), d.max(axis=0)
        rows = hi - lo + TB
        rows_up = (rows + ROWS_PER_DMA - 1) // ROWS_PER_DMA * ROWS_PER_DMA
        per_f = np.stack([pieces_per_wave(r) for r in rows.tolist()])     # [f][wave]
        pieces.update(np.unique(per_f).tolist())
        runs = runs or bool(np.any(per_f[1:] != per_f[:-1]))
        for ty in range(n_y):
            first = ty * TB + lo                                          # [f]: the window's first row
            in_time = (first >= 0) & (first + rows_up <= n_t)
            if np.any(first < 0):
                kinds.add("before_start")
            if np.any(first >= n_t):
                kinds.add("past_end")
            x = n_t - 1 - first                                           # a piece starts at the last row of the series
            if np.any((x >= 0) & (x % ROWS_PER_DMA == 0) & (x < rows)):
                kinds.add("straddle_end")
            for bg in range(n_bg):
                inside = in_time & ((bg + 1) * BEAMS <= n_b)
                if (bg + 1) * BEAMS > n_b:
                    kinds.add("partial_beams")
                if inside.any():
                    paths.add("inside")
                if not inside.all():
                    paths.add("lane")
                mixed = mixed or bool(inside.any() and not inside.all())
    return {"pairs": pairs, "pieces": pieces, "paths": paths, "lane_kinds": kinds, "mixed_tile": mixed, "piece_runs": runs}


def dedisperse_numpy(series, delays, n_t_out):
    """out[dm][t][b] = sum over ascending f of series[t + delays[dm][f]][f][b]: one np.float32 add per channel from +0; a row below
    0 or at or past n_t contributes nothing.  Written from the definition, not from the oracle's C."""
    series = np.asarray(series)
    assert series.dtype == np.float32
    n_t, n_f, n_b = series.shape
    delays = np.asarray(delays, np.int64)
    out = np.zeros((delays.shape[0], n_t_out, n_b), np.float32)
    t = np.arange(n_t_out, dtype=np.int64)[None, :]
    for f in range(n_f):
        row = t + delays[:, f][:, None]                                   # [dm][t]
        ok = (row >= 0) & (row < n_t)
        term = series[np.clip(row, 0, n_t - 1), f, :]                     # [dm][t][b]
        np.add(out, term, out=out, where=ok[:, :, None])
    return out


def make_series(seed, n_t, n_f, n_b):
    """rng.random * 10 ** uniform(0, 5) in float32: five decades, every row distinct -- a wrong row or another order changes bits."""
    rng = np.random.default_rng(seed)
    scale = (10.0 ** rng.uniform(0, 5, (n_t, n_f, n_b))).astype(np.float32)
    return (rng.random((n_t, n_f, n_b), dtype=np.float32) * scale).astype(np.float32)


class Case:
    """One input of the GPU tests: delays [n_dm][n_f] over a series [n_t][n_f][n_b] (made on demand from the seed), the output
    lengths it runs at, and what it claims about the paths it reaches (checked by tests/test_dm_paths_cpu.py against census)."""

    def __init__(self, name, n_t, n_b, delays, seed, extra_n_t_out=(), handle_n_freq=None, **claims):
        self.name, self.n_t, self.n_b, self.seed = name, n_t, n_b, seed
        self.delays = np.ascontiguousarray(delays, np.int32)
        assert np.array_equal(self.delays, delays)
        self.n_dm, self.n_f = self.delays.shape
        self.handle_n_freq = handle_n_freq      # a handle created at this channel count, its n_freq set afterwards (n_f beyond the fused kernel's contract)
        self.n_t_outs = sorted({n_t, max(1, n_t - int(self.delays.max()))} | set(extra_n_t_out))
        assert all(1 <= n <= n_t for n in self.n_t_outs)
        self.claims = claims                    # mask: the groups taken; pairs / pieces / paths / lane_kinds: subsets census must show; ...

    def series(self):
        return make_series(self.seed, self.n_t, self.n_f, self.n_b)

    @property
    def fits(self):
        return wide_fits(self.delays)

    @property
    def mask(self):
        return mask_of(self.fits)

    def census(self, n_t_out=None):
        """Over every output length the case runs at (or the one given): the union of what each reaches."""
        total = None
        for n in ([n_t_out] if n_t_out else self.n_t_outs):
            c = census(self.delays, self.n_t, n, self.n_b)
            if total is None:
                total = c
            else:
                total = {k: (v | c[k]) if isinstance(v, set) else (v or c[k]) for k, v in total.items()}
        return total

    def __repr__(self):
        return self.name


def _falling(n_f, top):
    """A base delay per channel that falls with f (channel 0 = the lowest frequency's longest delay)."""
    return np.linspace(top, 0, n_f).astype(np.int64)


# ---- 1. pair distance ------------------------------------------------------------------------------------------------------------
def pair_distances():
    """Every trial at base[f] + r, r independent in 0 .. 6: a wave's pair distance runs over -6 .. 6 and changes from channel to
    channel.  Both groups fit (span <= 6)."""
    rng = np.random.default_rng(101)
    n_f, n_dm = 48, 64
    delays = _falling(n_f, 30)[None, :] + rng.integers(0, 7, (n_dm, n_f))
    return Case("pair_distances", 200, 128, delays, 1, mask=0b11, pairs=set(PAIR_CLASSES), paths={"inside", "lane"})


PAIR_CONSTANT_D = (0, 1, 2, 3, 4, -1, -3)


def pair_constant_d(d):
    """Every pair of every group at distance d at every channel (trial A at base[f] + a, a in 0 .. 4 per wave and channel)."""
    rng = np.random.default_rng(200 + d)
    n_f, n_dm = 48, 64
    a = rng.integers(0, 5, (n_dm // 2, n_f))
    delays = np.empty((n_dm, n_f), np.int64)
    delays[0::2] = _falling(n_f, 30)[None, :] + 3 + a
    delays[1::2] = delays[0::2] + d
    cls = "<0" if d < 0 else ">=4" if d >= 4 else d
    return Case("pair_constant_d[%d]" % d, 160, 128, delays, 2, mask=0b11, pairs_exactly={cls})


# ---- 2. DMA pieces per wave, 3. the fit boundary -----------------------------------------------------------------------------------
def _group_with_spans(rng, base, spans):
    """32 trials, monotone in the trial, whose delays span exactly spans[f] at channel f (first trial at base, last at base + span)."""
    o = np.sort(rng.integers(0, np.asarray(spans)[None, :] + 1, (TRIALS, len(spans))), axis=0)
    o[0], o[-1] = 0, spans
    return base[None, :] + o


def piece_counts():
    """Five groups at 8 channels.  0: every trial at one delay (16 rows: waves 8 .. 15 issue nothing).  1 and 4: per channel a span out
    of {0, 15, 17, 47, 49, 79, 81, cap - 16}, shuffled: odd heights, and piece counts that change from window to window.  2: at the
    cap at every channel (4 pieces for waves 0 .. 3).  3: one row over the cap at ONE channel -- not taken, its neighbours are."""
    rng = np.random.default_rng(301)
    n_f = 8
    cap = rows_cap(n_f)
    menu = np.array([0, 15, 17, 47, 49, 79, 81, cap - TB])
    base = rng.integers(0, 10, n_f)
    over = np.array([0, 15, 17, 47, cap - 15, 79, 81, 3])
    groups = [_group_with_spans(rng, base, np.zeros(n_f, np.int64)), _group_with_spans(rng, base, rng.permutation(menu)),
              _group_with_spans(rng, base, np.full(n_f, cap - TB)), _group_with_spans(rng, base, over),
              _group_with_spans(np.random.default_rng(302), base, np.random.default_rng(303).permutation(menu))]
    return Case("piece_counts", 320, 128, np.concatenate(groups), 3, mask=0b10111, pieces={0, 1, 2, 3, 4}, piece_runs=True,
                paths={"inside", "lane"})


CAP_CHANNELS = (64, 256, 1024, 1025)


def cap_by_channels(n_f):
    """Group 0 spans rows_cap(n_f) - 16 at every channel (the three ring buffers full, behind tables of n_f channels); group 1 one row
    more at the LAST channel only.  1025 channels: the kernel is not launched at all."""
    rng = np.random.default_rng(400 + n_f)
    cap = rows_cap(min(n_f, MAX_FREQ))
    base = rng.integers(0, 4, n_f)
    at_cap = np.full(n_f, cap - TB)
    over = at_cap.copy()
    over[-1] += 1
    delays = np.concatenate([_group_with_spans(rng, base, at_cap), _group_with_spans(rng, base, over)])
    return Case("cap_by_channels[%d]" % n_f, 200, 4, delays, 4, handle_n_freq=256 if n_f > MAX_FREQ else None,
                mask=0b01 if n_f <= MAX_FREQ else 0)


# ---- 4. staging path ---------------------------------------------------------------------------------------------------------------
EDGE_BEAMS = (4, 124, 132, 256)


def edges(n_b):
    """Delays from -9 upwards over an odd number of rows: windows that begin before row 0, a two-row piece across the last row,
    windows wholly past the end (n_t_out = n_t), and beam tiles that are not full.  Also at n_t_out = 37 (no multiple of 16)."""
    n_f, n_dm = 40, 33
    delays = ((np.arange(n_dm)[:, None] + 3) * np.linspace(1.2, 0.0, n_f)[None, :]).astype(np.int64) - 9
    assert delays.min() == -9
    kinds = {"before_start", "past_end", "straddle_end"} | ({"partial_beams"} if n_b % BEAMS else set())
    full_tile = n_b >= BEAMS
    return Case("edges[%d]" % n_b, 151, n_b, delays, 5, extra_n_t_out=(37,), mask=0b11, lane_kinds=kinds,
                paths={"inside", "lane"} if full_tile else {"lane"}, mixed_tile=full_tile)


# ---- 5. ring tail, 6. trial counts -------------------------------------------------------------------------------------------------
FEW_CHANNELS = (1, 2, 3, 4, 5)


def few_channels(n_f):
    """1 .. 5 channels: the prologue alone, and both branches of the tail behind the loop over whole turns of the ring."""
    n_dm = 34
    delays = (np.arange(n_dm)[:, None] * np.linspace(1.0, 0.2, n_f)[None, :]).astype(np.int64)
    return Case("few_channels[%d]" % n_f, 120, 128, delays, 6, mask=0b11)


TRIAL_COUNTS = (1, 2, 31, 32, 33, 63)


def trial_counts(n_dm):
    """An odd number of trials (trial B of the last wave repeated, never stored), a last group of one trial, whole groups."""
    n_f = 24
    delays = (np.arange(n_dm)[:, None] * np.linspace(0.7, 0.0, n_f)[None, :]).astype(np.int64)
    return Case("trial_counts[%d]" % n_dm, 120, 64, delays, 7, mask=(1 << ((n_dm + TRIALS - 1) // TRIALS)) - 1)


def channels_multiple_of_64():
    """64 channels: dw_table_bytes has no padding, the look-ahead reads behind the last channel (tab[f + 3], offsAB[f + 1]) land in
    the first window buffer.  Steep ladder, so that what they read there differs from what a padded table would hold."""
    n_f, n_dm = 64, 64
    delays = (np.arange(n_dm)[:, None] * np.linspace(1.5, 0.0, n_f)[None, :]).astype(np.int64)
    return Case("channels_multiple_of_64", 180, 128, delays, 8, mask=0b11)


# ---- 7. stale flags ----------------------------------------------------------------------------------------------------------------
def _ladder(steps, n_f):
    return (np.cumsum(steps)[:, None] * np.linspace(1.0, 0.1, n_f)[None, :]).astype(np.int64)


def flag_ladders():
    """Four ladders over ONE series, run one after the other on one stream: each flips a group's verdict or shrinks the trial count
    against the call before it.  (96 trials, group 1 coarse) -> 0b101; (96, fine) -> 0b111; (32, coarse) -> 0; (64, fine) -> 0b11."""
    n_f, fine, coarse = 16, 0.5, 5.0
    ladders = [_ladder(np.concatenate([np.full(32, fine), np.full(32, coarse), np.full(32, fine)]), n_f), _ladder(np.full(96, fine), n_f),
               _ladder(np.full(32, coarse), n_f), _ladder(np.full(64, fine), n_f)]
    masks = [0b101, 0b111, 0, 0b11]
    n_t = 320
    common = n_t - int(ladders[0].max())                                # the output length all four run at in the test
    return [Case("flags_between_calls[%d]" % i, n_t, 128, d, 9, extra_n_t_out=(common,), mask=m) for i, (d, m) in enumerate(zip(ladders, masks))]


def stream_mixed_groups():
    """The mixed_groups ladder of test_gpu_round5's DM-stage test: group 0 fits a window, group 1 is far too coarse, group 2 fits.
    Returns (case, max_rows_per_push).  The stage's ring holds max_delay + 3 max_rows_per_push = 153 + 72 rows and a little more:
    the 320 rows of the series run past its seam by several pushes (the test asserts it against the capacity the stage reports)."""
    n_f = 32
    step = np.concatenate([np.full(32, 0.4), np.full(32, 4.0), np.full(32, 0.4)])
    delays = (np.cumsum(step)[:, None] * np.linspace(1.0, 0.05, n_f)[None, :]).astype(np.int32)
    return Case("stream_stage", 320, 132, delays, 10, mask=0b101), 24


def all_cases():
    """Every case of the GPU tests that runs through bf_dedisperse_dm_device."""
    return ([pair_distances()] + [pair_constant_d(d) for d in PAIR_CONSTANT_D] + [piece_counts()] + [cap_by_channels(n) for n in CAP_CHANNELS] +
            [edges(n) for n in EDGE_BEAMS] + [few_channels(n) for n in FEW_CHANNELS] + [trial_counts(n) for n in TRIAL_COUNTS] +
            [channels_multiple_of_64()] + flag_ladders() + [stream_mixed_groups()[0]])
