"""Plain CPU references of the audio encoder's non-GEMM kernels (csrc/frontend.hip, norm.hip,
cnn.hip, window_attention of attn.hip, swin.hip), one function per op, on the kernels' own layouts.

Pure torch / numpy on the CPU; every float is computed in ``dtype``: float64 is the reference,
float32 the yardstick (the same formula in the kernel's precision; its distance from the float64
run on a case's own data is what plain float32 arithmetic costs there).  ``round_to`` rounds to the
storage type where a kernel stores bf16.  The tolerance rule is mistral_ref.tolerance (4 x
yardstick + 1e-6, plus one bf16 step of the reference for a bf16 output); the two bf16 kernels
with internal rounding (window attention in bf16, the fused Swin block) use ``tolerance_bf16``:
max norm, 2 x the twin's largest deviation from float64.

Rounding points of the bf16 kernels, read from the sources and restated by the float32 twins:
  window_attn_mfma_kernel (attn.hip): q, k, v are bf16 inputs; scores, bias, mask, max and the
    row sum are f32 (the scale 1/sqrt(hd) multiplies the f32 score); P = exp(s - max), not yet
    normalised, is rounded to bf16 for the P V product (the row sum adds the unrounded P); the
    output (P V) / sum is rounded to bf16.
  window_attn_kernel<bf16> (VALU): q * scale, scores, softmax and P V in f32; only the output is
    rounded to bf16.
  swin_block_kernel (swin.hip): LN1 output -> bf16; q, k, v (+ bias) -> bf16; P -> bf16 and the
    attention output -> bf16 exactly as window_attn_mfma_kernel; proj + bias + residual stays f32;
    LN2 output -> bf16; GELU(fc1 + bias), the MLP hidden -> bf16; fc2 accumulates in f32 onto the
    residual.  Weights are bf16, biases, LayerNorm parameters and the bias table f32.

``mut`` names one deliberate, in-bounds arithmetic error of a kernel (MUTANTS).  It is only ever
set by tests/test_encoder_ref.py, which shows on the CPU that the inputs of the GPU cases tell
each of them from the reference by more than twice the case's tolerance.  No kernel is ever
altered.

The second half builds the inputs both test files share (cached: a case is built once).
"""
from __future__ import annotations

import functools
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mistral_ref import tolerance  # noqa: E402,F401  (the shared rule)

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
I32, I64 = torch.int32, torch.int64
NAN = float("nan")
NFFT, HOP, NMEL, NBIN = 1024, 320, 64, 513
WS = 8

MUTANTS = ("wa_hw_swap", "wa_roll_sign", "wa_thresh_swap", "wa_relpos_T", "wa_mask_shift0",
           "pm_part_swap", "lm_edge_repeat", "lm_pair_swap", "lm_stale_power",
           "ln_mean_ldx", "ln_rows_ident", "mp_div16", "head_axes", "conv_tap_T",
           "conv_no_border", "pool_odd_col", "w2i_no_clamp")


def _round(v, round_to):
    return v if round_to is None else v.to(round_to).to(v.dtype)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def tolerance_bf16(ref64, twin):
    """The bf16 kernels with internal rounding points: the kernel rounds where the twin rounds but
    sums in another order, so its error is another draw from the twin's error distribution.
    Max norm; -> (yardstick = max |twin - ref64|, tolerance = 2 x yardstick)."""
    yard = float((twin.double() - ref64).abs().max())
    return yard, 2.0 * yard


# ------------------------------------------------------------------ front end
def frame_index(T, mut=""):
    """[n_frames, 1024] sample index of every frame element after reflect padding by 512 (torch
    F.pad 'reflect': no edge repeat), n_frames = T // 320 + 1."""
    nf = T // HOP + 1
    o = torch.arange(nf)[:, None] * HOP - NFFT // 2 + torch.arange(NFFT)[None, :]
    if mut == "lm_edge_repeat":          # symmetric padding: the edge sample twice
        o = torch.where(o < 0, -o - 1, o)
        o = torch.where(o >= T, 2 * T - 1 - o, o)
    else:
        o = torch.where(o < 0, -o, o)
        o = torch.where(o >= T, 2 * (T - 1) - o, o)
    return o


def mel_power(wav, window, melW):
    """float64: wav [B, T] -> (mel power [B * n_frames, 64], bin power [B * n_frames, 513])."""
    B, T = wav.shape
    fr = wav.double()[:, frame_index(T)] * window.double()[None, None, :]
    spec = np.fft.rfft(fr.numpy(), axis=-1)
    pw = torch.from_numpy(spec.real ** 2 + spec.imag ** 2).reshape(-1, NBIN)
    return pw @ melW.double().t(), pw


def logmel(wav, window, melW, bn=None, dtype=F64, mut="", stride=0):
    """zs_logmel: wav [B, T] f32 -> [B * n_frames, 64]: reflect pad 512, Hann window, 1024-point
    DFT (float64: numpy rfft), power, mel matrix, 10 log10(max(., 1e-10)), optional bn0
    (bn = (mean, var, weight, bias), eps 1e-5).  The float32 twin is oracle.frontend.logmel (the
    windowed DFT as a float32 convolution).  ``stride`` (frames) is how far apart two iterations
    of a workgroup's frame loop are (lm_stale_power)."""
    B, T = wav.shape
    if dtype == F64:
        fr = wav.double()[:, frame_index(T, mut)] * window.double()[None, None, :]
        spec = np.fft.rfft(fr.numpy(), axis=-1)
        pw = torch.from_numpy(spec.real ** 2 + spec.imag ** 2).reshape(-1, NBIN)
        if mut == "lm_stale_power" and stride and pw.shape[0] > stride:
            pw = torch.cat([pw[:stride], pw[:pw.shape[0] - stride]])
        db = 10.0 * torch.log10(torch.clamp(pw @ melW.double().t(), min=1e-10))
        if mut == "lm_pair_swap":
            n2 = db.shape[0] // 2 * 2
            db = torch.cat([db[:n2].view(-1, 2, NMEL).flip(1).reshape(-1, NMEL), db[n2:]])
    else:
        from oracle import frontend as OF
        assert not mut
        db = OF.logmel(wav)[:, 0].reshape(-1, NMEL)
    if bn is not None:
        m, v, w, b = (t.to(dtype) for t in bn)
        db = (db - m) / torch.sqrt(v + 1e-5) * w + b
    return db


def _cubic(x, A=-0.75):
    c1 = lambda t: ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0
    c2 = lambda t: ((A * t - 5.0 * A) * t + 8.0 * A) * t - 4.0 * A
    return c2(x + 1.0), c1(x), c1(1.0 - x), c2((1.0 - x) + 1.0)


def wav2img(x, dtype=F64, mut=""):
    """zs_wav2img: x [B, T_in, 64] -> img [B, 256, 256]: bicubic (A = -0.75, align_corners) along
    time T_in -> 1024 (source index scale * t with scale = (T_in - 1) / 1023, taps i0 - 1 .. i0 + 2
    clamped to [0, T_in - 1]), then the fold img[chunk * 64 + mel][c] = resized[chunk * 256 + c][mel]."""
    B, T_in, _ = x.shape
    xd = x.to(dtype)
    t = torch.arange(1024, dtype=dtype)
    scale = torch.tensor(T_in - 1, dtype=dtype) / torch.tensor(1023, dtype=dtype)
    src = scale * t
    i0 = torch.floor(src)
    ws = _cubic(src - i0)
    i0 = i0.long()
    out = torch.zeros(B, 1024, 64, dtype=dtype)
    for k, w in enumerate(ws):
        idx = i0 - 1 + k
        if mut == "w2i_no_clamp":       # in bounds, but the neighbouring memory: wraps to the
            idx = idx % T_in            # other end of the clip instead of repeating the edge
        else:
            idx = idx.clamp(0, T_in - 1)
        out = out + xd[:, idx, :] * w[None, :, None]
    return out.view(B, 4, 256, 64).permute(0, 1, 3, 2).reshape(B, 256, 256)


def layernorm_rows(x, w, b, eps, dtype=F64):
    """Two-pass LayerNorm over the last axis."""
    xd = x.to(dtype)
    mean = xd.mean(-1, keepdim=True)
    d = xd - mean
    return d * torch.rsqrt((d * d).mean(-1, keepdim=True) + eps) * w.to(dtype) + b.to(dtype)


def patch_embed(img, w, bias, lnw, lnb, dtype=F64):
    """zs_patch_embed: img [B, 256, 256], w [96, 16] (k = ky * 4 + kx) -> [B * 4096, 96]:
    Conv2d(1 -> 96, k4 s4) + bias, LayerNorm(96, eps 1e-5); token = patch row * 64 + patch col."""
    B = img.shape[0]
    p = img.to(dtype).view(B, 64, 4, 64, 4).permute(0, 1, 3, 2, 4).reshape(B * 4096, 16)
    return layernorm_rows(p @ w.to(dtype).t() + bias.to(dtype), lnw, lnb, 1e-5, dtype)


def pack_clips(flat, off, lens, T):
    """zs_pack_clips: clip b = flat[off[b] : off[b] + lens[b]] cropped to T or zero-padded."""
    out = torch.zeros(len(lens), T)
    for b, (o, n) in enumerate(zip(off, lens)):
        n = min(int(n), T)
        out[b, :n] = flat[int(o):int(o) + n]
    return out


# ------------------------------------------------------------------ normalisation
def layernorm(x, M, C, ldx, rows, w, b, eps, dtype=F64, round_to=None, mut=""):
    """zs_layernorm: x a flat buffer of rows of pitch ldx; y[m] = LN(x[rows[m] or m][:C]).
    -> [M, C] (the caller lays it out with ldy)."""
    xv = x.view(-1, ldx)
    idx = torch.arange(M) if (rows is None or mut == "ln_rows_ident") else rows.long()
    xr = xv[idx].to(dtype)
    if mut == "ln_mean_ldx":
        mean = xr.mean(-1, keepdim=True)           # over the whole pitch: reads the tail
        d = xr[:, :C] - mean
        y = d * torch.rsqrt((d * d).mean(-1, keepdim=True) + eps) * w.to(dtype) + b.to(dtype)
    else:
        y = layernorm_rows(xr[:, :C], w, b, eps, dtype)
    return _round(y, round_to)


def patch_merge_ln(x, w, b, dtype=F64, round_to=None, mut=""):
    """zs_patch_merge_ln: x [B, H, W, C] -> [B * H/2 * W/2, 4C]: part p of output token (i, j) is
    x[2i + (p & 1), 2j + (p >> 1)]; LayerNorm(4C, eps 1e-5)."""
    B, H, W, C = x.shape
    parts = []
    for p in range(4):
        dy, dx = (p >> 1, p & 1) if mut == "pm_part_swap" else (p & 1, p >> 1)
        parts.append(x[:, dy::2, dx::2])
    g = torch.cat(parts, -1).reshape(-1, 4 * C)
    return _round(layernorm_rows(g, w, b, 1e-5, dtype), round_to)


def ln_meanpool(x, w, b, dtype=F64, mut=""):
    """zs_ln_meanpool: x [B, N, C] -> [B, C]: LayerNorm(C, eps 1e-5) per token, mean over N."""
    N = x.shape[1]
    s = layernorm_rows(x, w, b, 1e-5, dtype).sum(1)
    return s / (16 * math.ceil(N / 16) if mut == "mp_div16" else N)


def l2norm(x, eps, dtype=F64):
    xd = x.to(dtype)
    return xd / torch.clamp(torch.sqrt((xd * xd).sum(-1, keepdim=True)), min=eps)


def cast(x, dt):
    """zs_cast: round to nearest even (torch's own conversion)."""
    return x.to(dt)


# ------------------------------------------------------------------ CNN14
def conv3x3_bn_relu(x, w, scale, shift, dtype=F64, round_to=None, mut=""):
    """zs_conv3x3_bn_relu: x [B, H, W, Cin] NHWC, w [Cout, Kp] with k = (ky * 3 + kx) * Cin + ci
    (Cin = 1: 9 taps, padded to 32 with columns the kernel multiplies by zero activations), zero
    outside the image; relu(conv * scale + shift).  -> [B, H, W, Cout]."""
    B, H, W, Cin = x.shape
    xd = x.to(dtype)
    if mut == "conv_no_border":
        # no bounds test on the column: the flat pixel m + (ky - 1) W + (kx - 1) is read, which
        # at w = 0 / W - 1 is the end / start of the neighbouring image row (rows stay tested)
        flat = torch.nn.functional.pad(xd.reshape(B, H * W, Cin), (0, 0, W + 1, W + 1))
        taps = []
        for ky in range(3):
            for kx in range(3):
                s = (ky - 1) * W + (kx - 1) + W + 1
                taps.append(flat[:, s:s + H * W].reshape(B, H, W, Cin))
    else:
        xp = torch.nn.functional.pad(xd, (0, 0, 1, 1, 1, 1))
        order = [(kx, ky) for ky in range(3) for kx in range(3)] if mut == "conv_tap_T" else \
                [(ky, kx) for ky in range(3) for kx in range(3)]
        taps = [xp[:, ky:ky + H, kx:kx + W] for ky, kx in order]
    cols = torch.stack(taps, 3).reshape(B * H * W, 9 * Cin)
    y = cols @ w.to(dtype)[:, :9 * Cin].t()
    y = torch.relu(y * scale.to(dtype) + shift.to(dtype))
    return _round(y.view(B, H, W, -1), round_to)


def avgpool2(x, dtype=F64, round_to=None, mut=""):
    """zs_avgpool2: x [B, H, W, C] -> [B, H // 2, W // 2, C], (x00 + x01 + x10 + x11) / 4; an odd
    last row / column is dropped."""
    B, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    xd = x.to(dtype)
    if mut == "pool_odd_col" and W % 2:
        # the row pitch taken as 2 Wo: the odd last column joins the next row's windows
        flat = xd.reshape(B, H * W, C)[:, :H * 2 * Wo]
        xd = flat.reshape(B, H, 2 * Wo, C)
    xd = xd[:, :2 * Ho, :2 * Wo]
    s = (xd[:, 0::2, 0::2] + xd[:, 0::2, 1::2]) + xd[:, 1::2, 0::2] + xd[:, 1::2, 1::2]
    return _round(s / 4.0, round_to)


def cnn_head(x, dtype=F64, mut=""):
    """zs_cnn_head: x [B, H = time, W = mel, C] -> [B, C]: mean over W, then max + mean over H."""
    xd = x.to(dtype)
    if mut == "head_axes":
        m = xd.mean(1)
    else:
        m = xd.mean(2)
    return m.max(1).values + m.mean(1)


# ------------------------------------------------------------------ window attention
def window_tokens(B, H, W, shift, mut=""):
    """-> (tok [B * nWh * nWw, 64] natural token index of every window slot, reg [same] region
    label 0..8 of the slot's rolled coordinates).  Window (b, wy, wx), slot i = (iy, ix): rolled
    coordinates (sy, sx) = (8 wy + iy, 8 wx + ix), natural ((sy + shift) % H, (sx + shift) % W)
    (torch.roll by -shift); region row 0 / 1 / 2 for sy < H - 8 / < H - shift / else, the same for
    columns, label 3 ry + rx."""
    nWh, nWw = H // WS, W // WS
    n = nWh * nWw
    win = torch.arange(B * n)
    b, wyx = win // n, win % n
    if mut == "wa_hw_swap":
        wy, wx = wyx // nWh, wyx % nWh
    else:
        wy, wx = wyx // nWw, wyx % nWw
    i = torch.arange(64)
    sy = wy[:, None] * WS + (i // WS)[None, :]
    sx = wx[:, None] * WS + (i % WS)[None, :]
    sgn = -1 if mut == "wa_roll_sign" else 1
    hh, ww = (sy + sgn * shift) % H, (sx + sgn * shift) % W
    tok = (b[:, None] * H + hh) * W + ww

    def lab(y, n_):
        a, c = (n_ - shift, n_ - WS) if mut == "wa_thresh_swap" else (n_ - WS, n_ - shift)
        return torch.where(y < a, 0, torch.where(y < c, 1, 2))
    reg = lab(sy, H) * 3 + lab(sx, W)
    return tok, reg


def rel_index(mut=""):
    """[64, 64]: row of the bias table for (query i, key j): (iy - jy + 7) * 15 + (ix - jx + 7)."""
    i = torch.arange(64)
    dy = (i // WS)[:, None] - (i // WS)[None, :] + WS - 1
    dx = (i % WS)[:, None] - (i % WS)[None, :] + WS - 1
    idx = dy * (2 * WS - 1) + dx
    return idx.t().contiguous() if mut == "wa_relpos_T" else idx


def window_attention(qkv, B, H, W, C, heads, shift, table, dtype=F64, p_round=None,
                     out_round=None, mut=""):
    """zs_window_attention on token indices: qkv [B H W, 3C] and out [B H W, C] in natural token
    order.  Per window and head: softmax(q k^T / sqrt(hd) + table[rel_index] + mask) v with mask
    -100 between slots of different region labels (shift > 0 only).  ``p_round``: the MFMA
    kernel's rounding of the unnormalised exp(s - max) before P V (the row sum adds the unrounded
    values); ``out_round``: the stored output."""
    hd = C // heads
    tok, reg = window_tokens(B, H, W, shift, mut)
    nwin = tok.shape[0]
    g = qkv.to(dtype)[tok.reshape(-1)].view(nwin, 64, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = g[0], g[1], g[2]                                    # [nwin, heads, 64, hd]
    s = (q @ k.transpose(-1, -2)) * (hd ** -0.5)
    s = s + table.to(dtype)[rel_index(mut).reshape(-1)].view(64, 64, heads).permute(2, 0, 1)[None]
    if shift > 0 or mut == "wa_mask_shift0":
        if shift == 0:      # the mask of the shifted block (shift 4) applied to an unshifted one
            reg = window_tokens(B, H, W, WS // 2)[1]
        neq = reg[:, :, None] != reg[:, None, :]
        s = s + torch.where(neq, -100.0, 0.0).to(dtype)[:, None]
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    o = (_round(p, p_round) @ v) / p.sum(-1, keepdim=True)
    o = _round(o, out_round)                                       # [nwin, heads, 64, hd]
    out = torch.zeros(B * H * W, C, dtype=dtype)
    out[tok.reshape(-1)] = o.permute(0, 2, 1, 3).reshape(nwin * 64, C)
    return out


def softmax_stats(qkv, B, H, W, C, heads, shift, table):
    """float64 -> (scores [nwin, heads, 64, 64] with bias and mask, region labels [nwin, 64])."""
    hd = C // heads
    tok, reg = window_tokens(B, H, W, shift)
    nwin = tok.shape[0]
    g = qkv.double()[tok.reshape(-1)].view(nwin, 64, 3, heads, hd).permute(2, 0, 3, 1, 4)
    s = (g[0] @ g[1].transpose(-1, -2)) * (hd ** -0.5)
    s = s + table.double()[rel_index().reshape(-1)].view(64, 64, heads).permute(2, 0, 1)[None]
    if shift > 0:
        s = s + torch.where(reg[:, :, None] != reg[:, None, :], -100.0, 0.0)[:, None]
    return s, reg


def swin_block(x, sd, B, H, W, C, heads, shift, dtype=F64, rnd=None, mut="", name="blk."):
    """zs_swin_block: x [B H W, C] f32 -> x + proj(window_attention(LN1 x)), then + fc2(GELU(fc1(
    LN2 .))).  ``sd`` as tests/test_gpu_swin._block_sd (bf16-valued weights).  ``rnd`` = bf16 in
    the float32 twin: rounds at the kernel's rounding points (module docstring)."""
    f = lambda k: sd[name + k].to(dtype)
    xd = x.to(dtype)
    h = _round(layernorm_rows(xd, f("norm1.weight"), f("norm1.bias"), 1e-5, dtype), rnd)
    qkv = _round(h @ f("attn.qkv.weight").t() + f("attn.qkv.bias"), rnd)
    att = window_attention(qkv, B, H, W, C, heads, shift, f("attn.relative_position_bias_table"),
                           dtype, p_round=rnd, out_round=rnd, mut=mut)
    x1 = xd + att @ f("attn.proj.weight").t() + f("attn.proj.bias")
    h2 = _round(layernorm_rows(x1, f("norm2.weight"), f("norm2.bias"), 1e-5, dtype), rnd)
    hid = _round(torch.nn.functional.gelu(h2 @ f("mlp.fc1.weight").t() + f("mlp.fc1.bias")), rnd)
    return x1 + f("mlp.fc2.bias") + hid @ f("mlp.fc2.weight").t()


# ====================================================================== shared inputs
# ---- log-mel: (B, T, index of the exactly silent clip or None)
LOGMEL_T = 1920                        # 7 frames: 2-4 interior (fast path), 0, 1, 5, 6 reflect
LOGMEL_CASES = [(1, 1920, None), (5, 1920, 2), (900, 1920, 450), (1180, 1920, 7),
                (3, 513, None), (3, 640, 1)]
LOGMEL_WAVE_STRIDE = 2 * 4 * 768       # frames between two iterations of a wave (grid 768 x 4 pairs)
LOGMEL_BLOCK_STRIDE = 4 * 2048         # ... of a block of the block-per-4-frames kernel


@functools.lru_cache(maxsize=None)
def tables():
    """zsaac.frontend.make_tables on the CPU (window, twiddle, melW, mel_lo, mel_hi)."""
    from zsaac.frontend import make_tables
    return make_tables("cpu")


@functools.lru_cache(maxsize=None)
def logmel_wav(B, T, silent):
    """Seeded broadband clips that differ per clip: white noise of a per-clip level plus one tone
    per clip; clip ``silent`` is exactly zero."""
    g = gen(1000 * B + T)
    level = 0.05 + torch.rand(B, 1, generator=g)
    wav = torch.randn(B, T, generator=g) * level
    f = 200.0 + 6000.0 * torch.rand(B, 1, generator=g)
    wav = wav + 0.1 * level * torch.sin(2 * math.pi * f / 32000.0 * torch.arange(T)[None, :])
    if silent is not None:
        wav[silent] = 0.0
    return wav.float().contiguous()


def logmel_bn():
    g = gen(77)
    return (torch.randn(64, generator=g) * 5 - 20, torch.rand(64, generator=g) * 40 + 20,
            torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g))


@functools.lru_cache(maxsize=None)
def _logmel_base(B, T, silent):
    tb = tables()
    wav = logmel_wav(B, T, silent)
    return (logmel(wav, tb["window"], tb["melW"]), logmel(wav, tb["window"], tb["melW"], dtype=F32))


def logmel_refs(B, T, silent, with_bn):
    """-> (float64 reference, float32 twin) [B * n_frames, 64]; bn0 applied in each one's own
    precision."""
    r64, r32 = _logmel_base(B, T, silent)
    if not with_bn:
        return r64, r32
    m, v, w, b = logmel_bn()
    return ((r64 - m.double()) / torch.sqrt(v.double() + 1e-5) * w.double() + b.double(),
            (r32 - m) / torch.sqrt(v + 1e-5) * w + b)


# ---- wav2img / patch_embed
W2I_T = (2, 3, 1001, 1023, 1024)
W2I_B = (1, 3)


def w2i_case(B, T_in):
    return (torch.randn(B, T_in, 64, generator=gen(B + 10 * T_in)) * 5).contiguous()


def patch_embed_case(B):
    """The image is a ramp plus noise, so every token's 4 x 4 patch is distinct."""
    g = gen(40 + B)
    img = torch.randn(B, 256, 256, generator=g) + \
        (torch.arange(B * 65536, dtype=F32).view(B, 256, 256) % 8191) * 1e-3
    return dict(img=img.contiguous(), w=torch.randn(96, 16, generator=g) / 4,
                b=torch.randn(96, generator=g), lnw=1 + 0.2 * torch.randn(96, generator=g),
                lnb=torch.randn(96, generator=g))


# ---- pack_clips: (T, lengths, gap floats (NaN) after each clip)
def pack_case(T, lens, gaps):
    g = gen(2 + T)
    clips = [torch.randn(n, generator=g) for n in lens]
    parts, off, o = [], [], 0
    for c, gp in zip(clips, gaps):
        off.append(o)
        parts += [c, torch.full((gp,), NAN)]
        o += len(c) + gp
    return torch.cat(parts + [torch.full((4,), NAN)]), off


PACK_CASES = [(1000, [2500, 0, 7, 1000, 999, 1], [0, 0, 0, 0, 0, 0]),
              (4, [9, 3, 0, 4], [0, 0, 0, 0]),
              (1000, [1001, 5, 998, 1003], [2, 1, 3, 5])]     # offsets 1003, 1009, 2010: not % 4


# ---- layernorm: (name, C, M, ldx, ldy, kind)
LN_C = (4, 256, 260, 512, 768, 1024, 1028, 770, 1)
LN_M = (1, 5, 8)
LN_EPS = 1e-5
LN_ROWS = [6, 2, 2, 0, 6]              # a repeat, and the source's last row (7 rows)


def ln_cases():
    out = [(f"dense-C{C}-M{M}", C, M, C, C, "dense") for C in LN_C for M in LN_M]
    out += [(f"pad4-C{C}", C, 5, C + 4, C + 4, "dense") for C in (256, 768, 1028)]
    out += [("ldx+1-C256", 256, 5, 257, 256, "dense"), ("xoff-C512", 512, 5, 512, 512, "xoff"),
            ("yoff-C512", 512, 5, 512, 512, "yoff"), ("wboff-C512", 512, 5, 512, 512, "wboff"),
            ("rows-C768", 768, 5, 772, 768, "rows"), ("special-C768", 768, 8, 768, 768, "special")]
    return out


@functools.lru_cache(maxsize=None)
def ln_case(C, M, ldx, kind):
    """x: flat buffer of nrows rows of pitch ldx, NaN in the tails.  special: row 1 has mean 1e3
    and spread 1, row 2 is constant (eps decides: the output is b), row 3 has magnitude 1e-4."""
    g = gen(C * 31 + M * 7 + ldx)
    nrows = 7 if kind == "rows" else M
    x = torch.full((nrows, ldx), NAN)
    x[:, :C] = torch.randn(nrows, C, generator=g) * 2 + 0.5
    if kind == "special":
        x[1, :C] = 1e3 + torch.randn(C, generator=g)
        x[2, :C] = 3.25
        x[3, :C] *= 1e-4
    rows = torch.tensor(LN_ROWS, dtype=I32) if kind == "rows" else None
    return dict(x=x.reshape(-1).contiguous(), rows=rows,
                w=1 + 0.3 * torch.randn(C, generator=g), b=torch.randn(C, generator=g))


# ---- patch_merge_ln: (C, B, H, W)
PM_CASES = [(96, 1, 2, 2), (96, 3, 4, 8), (192, 3, 8, 4), (384, 1, 4, 8), (388, 3, 2, 2),
            (388, 1, 8, 4), (5, 3, 2, 2), (5, 1, 4, 8), (192, 1, 2, 2), (384, 3, 2, 2)]


def pm_case(C, B, H, W):
    g = gen(C + 3 * B + 5 * H + 7 * W)
    return dict(x=torch.randn(B, H, W, C, generator=g) * 2 + 0.3,
                w=1 + 0.3 * torch.randn(4 * C, generator=g), b=torch.randn(4 * C, generator=g))


# ---- ln_meanpool
MP_C = (48, 256, 260, 768, 772, 1024)
MP_N = (1, 15, 16, 17, 64)
MP_B = (1, 3)


def mp_case(B, N, C):
    g = gen(B + 3 * N + 5 * C)
    return dict(x=torch.randn(B, N, C, generator=g) * 2 + 0.3,
                w=1 + 0.3 * torch.randn(C, generator=g), b=torch.randn(C, generator=g))


def mp_max_c(lds_bytes):
    """The largest C zs_ln_meanpool accepts on a device with ``lds_bytes`` of LDS per workgroup:
    16 waves x C floats of partial sums, and the kernel's 32 values per lane (C <= 2048)."""
    return min(2048, lds_bytes // 64)


# ---- cast: values on a bf16 tie (exactly half way between two bf16 neighbours)
def cast_case(n):
    g = gen(n)
    x = torch.randn(n, generator=g) * 3
    ties = torch.tensor([0x3F808000, 0x3F818000, 0xBF808000, 0x40FF8000, 0x3F80FFFF, 0x3F808001,
                         0x00000000, 0x80000000, 0x7F7FFFFF], dtype=I64).to(I32).view(F32)
    k = min(n, ties.numel())
    x[:k] = ties[:k]
    return x


# ---- conv3x3
CONV_CH = [(1, 64), (64, 64), (64, 128), (32, 96), (32, 160), (128, 256)]
CONV_SHAPES = [(1, 1, 1), (1, 3, 5), (2, 21, 16), (3, 5, 9)]


@functools.lru_cache(maxsize=None)
def conv_case(Cin, Cout, B, H, W, dt):
    """x NHWC and packed weights as exact ``dt`` values; the shift is negative for about half the
    channels, so ReLU clips."""
    g = gen(Cin + 3 * Cout + 5 * B + 7 * H + 11 * W)
    x = torch.randn(B, H, W, Cin, generator=g).to(dt)
    w = (torch.randn(Cout, 9 * Cin, generator=g) / math.sqrt(9 * Cin)).to(dt)
    if Cin == 1:
        w = torch.nn.functional.pad(w, (0, 23))
    return dict(x=x.contiguous(), w=w.contiguous(), scale=torch.rand(Cout, generator=g) + 0.5,
                shift=torch.randn(Cout, generator=g) * 0.7)


POOL_SHAPES = [(2, 2), (21, 16), (16, 21), (5, 7)]
POOL_C = (1, 64)


def pool_case(H, W, C, dt, B=2):
    return torch.randn(B, H, W, C, generator=gen(H + 3 * W + 5 * C)).to(dt).contiguous()


HEAD_SHAPES = [(1, 1, 1), (31, 2, 2048), (7, 3, 300)]
HEAD_B = (1, 3)


def head_case(B, H, W, C, dt):
    """Mean -3: nearly every per-row mean is negative, a maximum initialised to 0 would show."""
    return (torch.randn(B, H, W, C, generator=gen(B + H + W + C)) - 3.0).to(dt).contiguous()


# ---- window attention: (B, H, W, heads, hd, shift)
WA_HW = [(8, 8), (8, 16), (16, 8), (16, 24)]
WA_SHIFT = (0, 4, 1, 7)


def wa_cases(hds):
    out = []
    for hd in hds:
        for (H, W) in WA_HW:
            for shift in WA_SHIFT:
                out.append((2 if H * W < 256 else 1, H, W, 2, hd, shift))
        out.append((1, 8, 8, 3, hd, 0))          # 3 (window, head) items: the MFMA block's tail
        out.append((1, 8, 8, 3, hd, 4))
    return out


@functools.lru_cache(maxsize=None)
def wa_case(B, H, W, heads, hd, shift, dt):
    """qkv as exact ``dt`` values (q, k scaled so the scores have a spread of a few units), bias
    table with spread +-3 (the bias decides some softmax rows)."""
    C = heads * hd
    g = gen(B + 3 * H + 5 * W + 7 * heads + 11 * hd + 13 * shift)
    qkv = torch.randn(B * H * W, 3 * C, generator=g)
    qkv[:, :2 * C] *= 1.5
    table = torch.rand(225, heads, generator=g) * 6 - 3
    return dict(qkv=qkv.to(dt).contiguous(), table=table, C=C)


# ---- fused Swin block: (C, B, H, W, shift)
SWIN_CASES = [(96, 1, 8, 8, 0), (96, 3, 8, 16, 4), (96, 1, 16, 8, 4), (192, 3, 8, 8, 4),
              (192, 1, 16, 8, 0), (192, 1, 8, 16, 4), (384, 1, 8, 8, 4), (384, 3, 16, 8, 0),
              (384, 1, 8, 16, 4), (96, 1, 8, 8, 4), (192, 1, 8, 8, 0), (384, 1, 8, 8, 0)]


def swin_x(C, B, H, W):
    return torch.randn(B * H * W, C, generator=gen(7 + C + B + H + 3 * W)).contiguous()
