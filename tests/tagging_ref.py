"""Plain CPU reference of the HTSAT tagging head (csrc/tagging.hip; htsat.py:830-894), on the
kernels' own layouts, in the style of tests/encoder_ref.py: every float is computed in ``dtype``
-- float64 is the reference, float32 the yardstick -- and ``rnd`` (torch.bfloat16) rounds where
the bf16 kernels round: xn, the conv's A operand, and the conv weight.  Nothing else is rounded:
``fine`` comes from the unrounded xn, products accumulate in f32, bias / sigmoid / mean are f32.

    x [B][64][C], token n = f * 8 + t (frequency row f, time column t)
    xn   = LayerNorm(x)                                   (eps 1e-5)
    tok(tau, c) = (2 (tau // 8) + c) * 8 + tau % 8        32 frames tau, 2 frequency bins c
    fine[b][tau] = (xn[b][tok(tau, 0)] + xn[b][tok(tau, 1)]) / 2
    z[b][tau][k] = bias[k] + sum_{c, d, ch} W[k][ch][c][d] xn[b][tok(tau + d - 1, c)][ch]
                   (zero where tau + d - 1 leaves [0, 32))
    frame = sigmoid(z), clip = sigmoid(mean_tau z)

Tolerances: f32 results and ``fine`` under encoder_ref.tolerance (4 x the float32 yardstick +
1e-6), bf16 results under encoder_ref.tolerance_bf16 (2 x the rounding twin's deviation).

``mut`` names one deliberate arithmetic error (MUTANTS); it is only ever set by
tests/test_tagging_ref.py, which shows that the GPU cases' inputs tell each from the reference.
The second half builds the inputs the CPU and GPU test files share (cached).
"""
from __future__ import annotations

import functools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from encoder_ref import (F32, F64, BF16, _round, gen, layernorm_rows, tolerance,  # noqa: E402,F401
                         tolerance_bf16)

FRAMES, BINS, TAPS = 32, 2, 3
FRAME_SECONDS = 0.32          # 1024 spectrogram frames over 10.24 s, divided by 32

MUTANTS = ("pad_group", "bin_swap", "tap_rev", "tau_4t_g", "mean_sigmoid", "fine_bf16")


def tok(tau, c, mut=""):
    """The token of time frame tau, frequency bin c (htsat.py:834-839)."""
    if mut == "tau_4t_g":
        g, t = tau % 4, tau // 4
    else:
        g, t = tau // 8, tau % 8
    return (2 * g + c) * 8 + t


def weight_matrix(W, mut=""):
    """tscam_conv.weight [N][C][2][3] -> [N][6C], column (c * 3 + d) * C + ch."""
    if mut == "tap_rev":
        W = W.flip(3)
    return W.permute(0, 2, 3, 1).reshape(W.shape[0], -1)


def gather(xn, mut=""):
    """xn [B][64][C] -> the conv's A operand [B][32][6C] (the reference materialises what the
    kernel gathers): column block (c, d) of frame tau is token tok(tau + d - 1, c), or zero."""
    B, _, C = xn.shape
    A = torch.zeros(B, FRAMES, BINS * TAPS * C, dtype=xn.dtype)
    for tau in range(FRAMES):
        for c in range(BINS):
            for d in range(TAPS):
                ts = tau + d - 1
                ok = 0 <= ts < FRAMES
                if mut == "pad_group":
                    ok = ok and ts // 8 == tau // 8
                if ok:
                    cc = 1 - c if mut == "bin_swap" else c
                    k0 = (c * TAPS + d) * C
                    A[:, tau, k0:k0 + C] = xn[:, tok(ts, cc, mut)]
    return A


def head(x, lnw, lnb, W, bias, dtype=F64, rnd=None, mut=""):
    """-> dict(xn [B][64][C] (rounded to ``rnd``), fine [B][32][C], z, frame [B][32][N],
    clip [B][N]), all in ``dtype``."""
    xn = layernorm_rows(x, lnw, lnb, 1e-5, dtype)
    xr = _round(xn, rnd)
    src = _round(xn, BF16) if mut == "fine_bf16" else xn
    t0 = [tok(tau, 0, mut) for tau in range(FRAMES)]
    t1 = [tok(tau, 1, mut) for tau in range(FRAMES)]
    fine = (src[:, t0] + src[:, t1]) / 2
    Wm = _round(weight_matrix(W, mut).to(dtype), rnd)
    z = gather(xr, mut) @ Wm.t() + bias.to(dtype)
    frame = torch.sigmoid(z)
    clip = frame.mean(1) if mut == "mean_sigmoid" else torch.sigmoid(z.mean(1))
    return dict(xn=xr, fine=fine, z=z, frame=frame, clip=clip)


def topk(v, k):
    """Per row of v [B][N]: the k largest, value descending, ties to the lower index ->
    (values [B][k], indices [B][k] int64); rows shorter than k are filled with (-inf, 0x7fffffff)
    (zs_sim_topk_finalize's padding)."""
    B, N = v.shape
    vals = torch.full((B, k), float("-inf"), dtype=v.dtype)
    idx = torch.full((B, k), 0x7fffffff, dtype=torch.int64)
    for b in range(B):
        order = sorted(range(N), key=lambda n: (-float(v[b, n]), n))[:k]
        for q, n in enumerate(order):
            vals[b, q], idx[b, q] = v[b, n], n
    return vals, idx


def segments(probs32, threshold, min_frames=1):
    """The maximal runs of frames with probability >= threshold that are at least ``min_frames``
    long, as (first frame, one past the last frame, peak) -- restated here independently of
    zsaac.tagging.segments."""
    out, start = [], None
    p = [float(v) for v in probs32]
    for i, v in enumerate(p + [float("-inf")]):
        if v >= threshold:
            start = i if start is None else start
        elif start is not None:
            if i - start >= min_frames:
                out.append((start, i, max(p[start:i])))
            start = None
    return out


# ------------------------------------------------------------------ the shared cases
CASE_B = (1, 3)
CASE_C = (32, 768)
CASE_N = (1, 16, 17, 527)
CASES = [(B, C, N) for B in CASE_B for C in CASE_C for N in CASE_N]


def ldf_of(N, padded):
    return N + 5 if padded else N


@functools.lru_cache(maxsize=None)
def case(B, C, N):
    """x: tokens with a mean and a spread per token; W scaled so that z has a spread of about 1.5
    (sigmoid neither saturated nor linear) and a per-class trend over time (mean of sigmoids and
    sigmoid of the mean differ)."""
    g = gen(1000 * B + 7 * C + N)
    x = torch.randn(B, 64, C, generator=g) * (1 + torch.rand(B, 64, 1, generator=g)) + 0.3
    lnw = 1 + 0.3 * torch.randn(C, generator=g)
    lnb = 0.5 * torch.randn(C, generator=g)
    W = torch.randn(N, C, 2, 3, generator=g) * (1.5 / (6 * C) ** 0.5)
    bias = torch.randn(N, generator=g)
    return dict(x=x, lnw=lnw, lnb=lnb, W=W, bias=bias)


@functools.lru_cache(maxsize=None)
def case_refs(B, C, N):
    """(float64 reference, float32 yardstick, bf16-rounding twin in float32) of a case."""
    c = case(B, C, N)
    a = (c["x"], c["lnw"], c["lnb"], c["W"], c["bias"])
    return head(*a), head(*a, dtype=F32), head(*a, dtype=F32, rnd=BF16)


@functools.lru_cache(maxsize=None)
def dup_case():
    """B = 2, C = 32, N = 150: rows 3 and 140 of the weight (and of the bias) are equal -- n-tiles
    0 and 8, different waves and different workgroups -- and so are rows 20 and 21."""
    c = dict(case(2, 32, 150))
    W, bias = c["W"].clone(), c["bias"].clone()
    W[140], bias[140] = W[3], bias[3]
    W[21], bias[21] = W[20], bias[20]
    c["W"], c["bias"] = W, bias
    return c
