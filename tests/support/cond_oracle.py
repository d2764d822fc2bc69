"""numpy restatement of the conditioning stage (docs/CONDITIONING.md section 1): push totals in segments of 32 rows, the window,
the channel summary in the OSUM order, the mask with its two lower medians, the fp32 apply and the zero-DM subtraction.  Every
operation is one IEEE operation on arrays (numpy never fuses a multiply with an add).  No GPU, no libdsabf."""
from __future__ import annotations

import numpy as np

SEGMENT = 32


def push_totals(x):
    """fp64 sum and sum of squares per (f, b) of the rows x [n][f][b]: segments of 32 rows, each from +0.0 in ascending t, the
    segments added in ascending order from +0.0."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    S, Q = np.zeros(x64.shape[1:]), np.zeros(x64.shape[1:])
    for t0 in range(0, x64.shape[0], SEGMENT):
        s, q = np.zeros_like(S), np.zeros_like(Q)
        for t in range(t0, min(t0 + SEGMENT, x64.shape[0])):
            s = s + x64[t]
            q = q + x64[t] * x64[t]                    # (double)x (double)x: exact
        S, Q = S + s, Q + q
    return S, Q


def osum(v):
    """OSUM over the last axis (docs/CALIBRATION.md section 2, any n): 64 partial sums from +0.0, partial l adds the indices
    l, l + 64, ... ascending; then six halving steps p[l] = p[l] + p[l + w], w = 32, 16, ..., 1."""
    v = np.asarray(v, np.float64)
    p = np.zeros(v.shape[:-1] + (64,))
    for i in range(v.shape[-1]):
        p[..., i % 64] = p[..., i % 64] + v[..., i]
    w = 32
    while w >= 1:
        p = p[..., :w] + p[..., w:2 * w]
        w //= 2
    return p[..., 0]


def lower_median(v):
    """Element (m - 1) // 2 of the m sorted values."""
    v = np.sort(np.asarray(v, np.float64))
    return v[(v.size - 1) // 2]


class Conditioner:
    """The stage: push(x [n][f][b] float32) returns the conditioned rows; .mask (uint8 [f]), .n_good are those of the last push."""

    def __init__(self, n_freq_total, n_beams, baseline_pushes=8, zero_dm=True, auto_threshold=0.0, mask=None):
        self.F, self.B, self.W, self.zero_dm = n_freq_total, n_beams, baseline_pushes, bool(zero_dm)
        self.k = float(auto_threshold) * 1.4826
        self.static = np.zeros(n_freq_total, np.uint8)
        if mask is not None:
            self.set_mask(mask)
        self.window = []
        self.mask, self.n_good = np.zeros(n_freq_total, np.uint8), n_freq_total

    def set_mask(self, mask):
        self.static = (np.asarray(mask) != 0).astype(np.uint8)
        assert self.static.shape == (self.F,)

    def push(self, x):
        x = np.ascontiguousarray(x, np.float32)
        assert x.ndim == 3 and x.shape[1:] == (self.F, self.B) and x.shape[0] >= 1
        # (a), (b)
        self.window = (self.window + [(x.shape[0],) + push_totals(x)])[-self.W:]
        S, Q, n = np.zeros((self.F, self.B)), np.zeros((self.F, self.B)), 0
        for wn, ws, wq in self.window:                 # oldest first
            S, Q, n = S + ws, Q + wq, n + wn
        mu = S / float(n)
        mm = mu * mu
        var = Q / float(n) - mm
        live = var > mm * 2.0 ** -40
        with np.errstate(invalid="ignore", divide="ignore"):
            r32 = np.where(live, (1.0 / np.sqrt(np.where(live, var, 1.0))).astype(np.float32), np.float32(0.0)).astype(np.float32)
        mu32 = mu.astype(np.float32)
        # (c)
        cm = osum(mu) / float(self.B)
        cv = osum(np.where(var > 0.0, var, 0.0)) / float(self.B)
        mask = (self.static != 0) | ~((cm > 0.0) & (cv > 0.0))
        if self.k > 0.0 and np.any(~mask):
            elig = ~mask
            q = cv[elig] / (cm[elig] * cm[elig])
            med = lower_median(q)
            mad = lower_median(np.abs(q - med))
            if mad > 0.0:
                hit = np.zeros(self.F, bool)
                hit[elig] = q > med + self.k * mad
                mask = mask | hit
        self.mask = mask.astype(np.uint8)
        self.n_good = int(np.count_nonzero(~mask))
        # (d)
        zero = mask[None, :, None] | ~live[None, :, :]
        y = np.where(zero, np.float32(0.0), (x - mu32[None]) * r32[None]).astype(np.float32)
        # (e)
        if self.zero_dm and self.n_good:
            inv = np.float32(1.0 / float(self.n_good))
            z = np.zeros((x.shape[0], self.B), np.float32)
            for f in np.flatnonzero(~mask):            # ascending, sequential, fp32
                z = z + y[:, f, :]
            z = z * inv
            y = np.where(mask[None, :, None], np.float32(0.0), y - z[:, None, :]).astype(np.float32)
        return y
