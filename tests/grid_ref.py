"""Plain CPU references of the grid decode's phases (csrc/decode_grid.hip: zs_gpt2_decode_persist /
_phases and their f32 twins), one function per phase, and the cases the GPU tests run.

Pure torch on the CPU; every float is computed in ``dtype``: float64 is the reference and uses the
textbook definition (LayerNorm, then a linear layer; a softmax over all keys; HF's tanh gelu; an
argmax), float32 is the yardstick and uses the kernel's documented formula and order (the header
comment of decode_grid.hip): a GEMM element as four K-quarter partial sums added (p0 + p1) + (p2 +
p3), LayerNorm statistics in one pass over the bf16 pairs (sum x and sum x^2 per lane, the row's 4
lanes, the 4 waves), the fold rstd (x W' - mean cs) + b', the online softmax in 32-key chunks
(started from the step's own key, as phase_b does).  The f32 parity kernels normalise in two
passes and multiply afterwards; a reference called without column sums (``cs=None``) follows them.
The rule is mistral_ref.tolerance: 4 x yardstick + 1e-6, a bf16 output adds 2^-8 |ref|.

Operands are taken in their storage type (bf16 or f32) and widened.  Nothing here comes from
running a kernel, from a golden or from the original project.  tests/test_grid_ref.py ties these
functions to torch's own layer_norm / softmax / gelu / linear / argmax, checks the host fold of
Gpt2Weights and asserts the input conditions of the GPU cases; tests/test_gpu_grid_kernels.py
compares the kernels with them, one phase launch at a time.

``mut`` names one deliberate, in-bounds arithmetic error (MUTANTS).  It is only ever set by
tests/test_grid_ref.py, which shows on the CPU that the inputs of the GPU cases tell each of them
from the reference by more than twice the case's tolerance.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import glue_ref
from gemm_ref import act_apply
from mistral_ref import tolerance  # noqa: F401  (the one rule, re-exported)

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
I32 = torch.int32
D, NH, HD, DFF, NLY, RM = 768, 12, 64, 3072, 12, 64
QKVN = 3 * D
EPS = 1e-5
LAUNCHES = 62                # per step: 5 l + {A, B, C, D, E}, F = 60, the bookkeeping = 61
PH = dict(A=0, B=1, C=2, D=3, E=4)
SENT = -776.0                # exact in bf16; no case's output comes near it

MUTANTS = ("cs_unrounded", "eps_dropped", "scale_dropped", "new_key_dropped",
           "chunk_tail_dropped", "gelu_erf", "resid_from_xb", "kv_slot_off_by_one", "tie_high",
           "temp_mul", "pad_column_wins")


def row_tolerance(ref64, ref32, bf16=False):
    """mistral_ref.tolerance row by row (each row of a phase is a problem of its own: its
    LayerNorm, its attention, its residual): never wider than the rule over the whole tensor.
    The references are the unrounded results; ``bf16`` adds the output's own rounding step.
    -> (the largest row yardstick, tolerance tensor like ref64)."""
    yard = (ref32.double() - ref64).abs().reshape(ref64.shape[0], -1).max(-1).values
    tol = (4.0 * yard + 1e-6).reshape(-1, *([1] * (ref64.dim() - 1))).expand_as(ref64).clone()
    if bf16:
        tol = tol + ref64.abs() * 2.0 ** -8
    return float(yard.max()), tol


def launch(layer, phase):
    """Launch index of phase 'A' .. 'E' of block ``layer``, 'F' or 'book'."""
    return 60 if phase == "F" else 61 if phase == "book" else 5 * layer + PH[phase]


# ------------------------------------------------------------------ workspace layout (mirrored)
# The constexpr int WS_* of decode_grid.hip; tests/test_grid_ref.py reads the source and compares.
WS_SYNC_BYTES = 4096
WS_KEY = 8 * 128 + 128       # after the 8 barrier shards and the timeout word: u64 [2][64]


def ws_layout(mode):
    """Byte offsets of the hand-off regions behind the sync page -> dict (Q, ATT, XB, HID, X (bf16
    mode only), BYTES)."""
    e = 2 if mode == "bf16" else 4
    o = dict(Q=WS_SYNC_BYTES)
    o["ATT"] = o["Q"] + RM * D * e
    o["XB"] = o["ATT"] + RM * D * e
    o["HID"] = o["XB"] + RM * D * e
    if mode == "bf16":
        o["X"] = o["HID"] + RM * DFF * e
        o["BYTES"] = o["X"] + RM * D * 4
    else:
        o["BYTES"] = o["HID"] + RM * DFF * e
    return o


# ------------------------------------------------------------------ fragment order
def frag_index(nrows, K, width):
    """Flat index of element (row, col) in the MFMA fragment order [nrows / 16][K / (4 width)][64]
    [width] (width 8: bf16, 4: f32): row block row >> 4, k-step col / (4 width), lane (row & 15) +
    16 ((col / width) & 3), element col % width (decode_grid.hip frag_off / ldw).  -> int64
    [nrows, K]."""
    assert nrows % 16 == 0 and K % (4 * width) == 0
    row = torch.arange(nrows).view(-1, 1)
    col = torch.arange(K).view(1, -1)
    ks = K // (4 * width)
    lane = (row & 15) + 16 * ((col // width) & 3)
    return (((row >> 4) * ks + col // (4 * width)) * 64 + lane) * width + col % width


def frag_pack(x, nrows=None, fill=0.0):
    """x [n, K] (bf16 or f32) -> fragment order, flat [nrows K]; rows past n hold ``fill``."""
    n, K = x.shape
    nrows = -(-n // 16) * 16 if nrows is None else nrows
    width = 8 if x.dtype == BF16 else 4
    full = torch.full((nrows, K), fill, dtype=x.dtype)
    full[:n] = x
    out = torch.empty(nrows * K, dtype=x.dtype)
    out[frag_index(nrows, K, width).reshape(-1)] = full.reshape(-1)
    return out


def frag_unpack(buf, nrows, K):
    """Fragment order (flat or shaped) -> [nrows, K]."""
    width = 8 if buf.dtype == BF16 else 4
    return buf.reshape(-1)[frag_index(nrows, K, width)]


def key_decode(keys):
    """64-bit argmax keys (int64 tensor: order-preserving logit bits << 32 | ~id) -> (logit f32
    [n], id int64 [n])."""
    k = keys.numpy().astype(np.uint64)
    hi = (k >> np.uint64(32)).astype(np.uint32)
    u = np.where(hi & np.uint32(0x80000000), hi & np.uint32(0x7fffffff), ~hi).astype(np.uint32)
    ids = (~(k & np.uint64(0xffffffff)).astype(np.uint32)).astype(np.int64)
    return torch.from_numpy(u.view(np.float32).copy()), torch.from_numpy(ids)


# ------------------------------------------------------------------ arithmetic
def _store(v, out_dtype):
    """Round to the storage type of a hand-off (bf16), or keep (f32 / None)."""
    return v.to(F32).to(BF16).to(v.dtype) if out_dtype == BF16 else v


def matmul_q(a, w, dtype=F64, kstep=32):
    """a w^T, operands widened to ``dtype``.  float64: one product.  float32: the four K quarters
    apart, each accumulated over its k-steps from 0 upwards, added (p0 + p1) + (p2 + p3)."""
    a, w = a.to(dtype), w.to(dtype)
    if dtype == F64:
        return a @ w.t()
    K = a.shape[1]
    q = K // 4
    p = []
    for v in range(4):
        acc = torch.zeros(a.shape[0], w.shape[0], dtype=dtype)
        for k in range(v * q, (v + 1) * q, kstep):
            acc = acc + a[:, k:k + kstep] @ w[:, k:k + kstep].t()
        p.append(acc)
    return (p[0] + p[1]) + (p[2] + p[3])


def _lane_sums(v, width):
    """Sum over a [R, 768] float32 row in the kernels' order: lane (wave w, group g) adds its
    ``width`` columns of each of its k-steps pairwise and in increasing order, then the row's 4
    lanes (l0 + l1) + (l2 + l3), then the waves (w0 + w1) + (w2 + w3).  -> [R, 1]."""
    R = v.shape[0]
    n = D // (16 * width)
    t = v.reshape(R, 4, n, 4, width // 2, 2)
    acc = torch.zeros(R, 4, 4, dtype=v.dtype)
    for i in range(n):
        pr = t[:, :, i, :, :, 0] + t[:, :, i, :, :, 1]
        if width == 8:
            for j in range(4):
                acc = acc + pr[..., j]
        else:
            acc = acc + (pr[..., 0] + pr[..., 1])
    ln = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])
    return ((ln[:, 0] + ln[:, 1]) + (ln[:, 2] + ln[:, 3])).unsqueeze(-1)


def ln_stats(x, dtype=F64, onepass=False, mut=""):
    """Mean and 1 / sqrt(var + 1e-5) of each row (biased variance).  float64: the definition.
    float32 ``onepass``: var = E[x^2] - mean^2 from the sums in the bf16 kernel's order, clamped at
    0; float32 otherwise: the f32 kernel's two passes."""
    eps = 0.0 if mut == "eps_dropped" else EPS
    x = x.to(dtype)
    if dtype == F64:
        mean = x.mean(-1, keepdim=True)
        d = x - mean
        return mean, torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    inv = torch.tensor(1.0 / D, dtype=dtype)
    if onepass:
        mean = _lane_sums(x, 8) * inv
        ex2 = _lane_sums(x * x, 8) * inv
        return mean, torch.rsqrt(torch.clamp_min(ex2 - mean * mean, 0.0) + eps)
    mean = _lane_sums(x, 4) * inv
    d = x - mean
    return mean, torch.rsqrt(_lane_sums(d * d, 4) * inv + eps)


def ln_linear(x, w, bias, cs=None, dtype=F64, kstep=32, ln=None, mut="", cs_mut=None):
    """LayerNorm(x) w^T + bias, x [R, 768] and w [N, 768] in their storage types, bias [N] f32.
    ``ln`` = (g, beta): the LayerNorm's own affine (unfolded weights; float64 only), else it only
    normalises (the affine is folded into w and bias).  float32 with ``cs`` (the column sums of
    w): the bf16 kernel's fold rstd (x w^T - mean cs) + bias on one-pass statistics; float32
    without: the f32 kernel's normalise (two passes), then multiply."""
    if mut == "cs_unrounded":            # the fold with column sums of the weights before rounding
        mean, rstd = ln_stats(x, F64)
        return rstd * (matmul_q(x, w, F64) - mean * cs_mut.to(F64)) + bias.to(F64)
    if dtype == F64:
        mean, rstd = ln_stats(x, F64, mut=mut)
        y = (x.to(F64) - mean) * rstd
        if ln is not None:
            y = y * ln[0].to(F64) + ln[1].to(F64)
        return y @ w.to(F64).t() + bias.to(F64)
    assert ln is None and not mut
    if cs is None:
        mean, rstd = ln_stats(x, dtype)
        return matmul_q((x.to(dtype) - mean) * rstd, w, dtype, kstep) + bias.to(dtype)
    mean, rstd = ln_stats(x, dtype, onepass=True)
    return rstd * (matmul_q(x, w, dtype, kstep) - mean * cs.to(dtype)) + bias.to(dtype)


def embed_sum(wte, wpe, tok, pos):
    """The residual stream entering block 0: f32(wte[tok]) + f32(wpe[pos]), one f32 rounding (none
    for bf16 tables: the sum of two bf16 values of like magnitude fits f32)."""
    return wte[tok.long()].to(F32) + wpe[pos.long()].to(F32)


# ------------------------------------------------------------------ the phases
def phase_a(x, w, bias, cs, kc, vc, pos, dtype=F64, out_dtype=BF16, kstep=32, ln=None, mut="",
            cs_mut=None):
    """A: ln_1 + c_attn.  x [R, 768] the LayerNorm's input rows (layer 0: bf16(embed_sum), f32
    mode: embed_sum).  -> (q [R, 768], kc', vc'): the caches [>= R][12][Lmax][64] widened to
    ``dtype`` with k / v written at slot pos[row] of each head, everything rounded to
    ``out_dtype`` where that is bf16."""
    R = x.shape[0]
    y = _store(ln_linear(x, w, bias, cs, dtype, kstep, ln, mut, cs_mut), out_dtype)
    kc2, vc2 = kc.to(dtype).clone(), vc.to(dtype).clone()
    Lmax = kc.shape[2]
    for r in range(R):
        p = int(pos[r])
        if mut == "kv_slot_off_by_one":
            p = p + 1 if p + 1 < Lmax else p - 1
        kc2[r, :, p] = y[r, D:2 * D].view(NH, HD)
        vc2[r, :, p] = y[r, 2 * D:].view(NH, HD)
    return y[:, :D], kc2, vc2


def phase_b(q, kc, vc, pos, dtype=F64, out_dtype=BF16, mut=""):
    """B: per (row, head) softmax(q . K[0 .. pos] / 8) V[0 .. pos]; the caches hold the step's own
    key / value at slot pos.  -> att [R, 768] (head h in columns 64 h .. + 64)."""
    assert not mut or dtype == F64
    R = q.shape[0]
    out = torch.zeros(R, D, dtype=dtype)
    for r in range(R):
        p = int(pos[r])
        qh = q[r].to(dtype).view(NH, HD)
        K, V = kc[r, :, :p + 1].to(dtype), vc[r, :, :p + 1].to(dtype)
        s = torch.einsum("hd,hjd->hj", qh, K)
        if mut != "scale_dropped":
            s = s * 0.125
        if dtype == F64:
            keep = torch.ones(p + 1, dtype=torch.bool)
            if mut == "new_key_dropped":
                keep[p] = False
            if mut == "chunk_tail_dropped":          # the keys past the last full 32 of the cache
                keep[32 * (p // 32):p] = False
            s, V = s[:, keep], V[:, keep]
            e = torch.exp(s - s.max(-1, keepdim=True).values)
            o = torch.einsum("hj,hjd->hd", e / e.sum(-1, keepdim=True), V)
        else:
            m, tot, o = s[:, p].clone(), torch.ones(NH, dtype=dtype), V[:, p].clone()
            for c0 in range(0, p, 32):
                c1 = min(c0 + 32, p)
                mn = torch.maximum(m, s[:, c0:c1].max(-1).values)
                scale = torch.exp(m - mn)
                e = torch.exp(s[:, c0:c1] - mn[:, None])
                tot = tot * scale + e.sum(-1)
                o = o * scale[:, None] + torch.einsum("hj,hjd->hd", e, V[:, c0:c1])
                m = mn
            o = o * (1.0 / tot)[:, None]
        out[r] = o.reshape(D)
    return _store(out, out_dtype)


def phase_ce(a, w, bias, x_old, dtype=F64, kstep=32, mut=""):
    """C / E: x_new = (a w^T + bias) + x_old; a [R, K] in its storage type, x_old [R, 768] the
    residual stream (f32; block 0's C: embed_sum).  -> x_new in ``dtype`` (xb_of: its bf16 copy)."""
    xo = x_old.to(F32).to(BF16) if mut == "resid_from_xb" else x_old
    return (matmul_q(a, w, dtype, kstep) + bias.to(dtype)) + xo.to(dtype)


def xb_of(x):
    """The bf16 copy of the f32 residual stream (round to nearest even)."""
    return x.to(F32).to(BF16)


def phase_d(x, w, bias, cs, dtype=F64, out_dtype=BF16, kstep=32, ln=None, mut="", cs_mut=None):
    """D: gelu_new(ln_2(x) w^T + bias) -> (hid [R, 3072], the pre-activations)."""
    h = ln_linear(x, w, bias, cs, dtype, kstep, ln, mut, cs_mut)
    if dtype == F64:
        g = act_apply(h, "gelu_erf" if mut == "gelu_erf" else "gelu_tanh")
    elif cs is not None:         # gelu_new_fast: 0.5 (1 + tanh u) = 1 / (1 + exp(-2 u))
        g = h * (1.0 / (1.0 + torch.exp(-1.5957691216057308 * (h + (0.044715 * h * h) * h))))
    else:
        g = act_apply(h, "gelu_tanh")
    return _store(g, out_dtype), h


def phase_f(x, w, bias, cs, V, temperature=1.0, dtype=F64, kstep=32, ln=None, mut=""):
    """F: logits[v] = ln_f(x) . w[v] + bias[v], divided by the temperature; w [16 ceil(V / 16),
    768] (rows past V zero), bias likewise.  -> (logits [R, V], per row the largest value and the
    lowest id attaining it)."""
    lg = ln_linear(x, w, bias, cs, dtype, kstep, ln)
    if temperature != 1.0:
        t = torch.tensor(temperature, dtype=F32).to(dtype)
        lg = lg * t if mut == "temp_mul" else lg / t
    n = lg.shape[1] if mut == "pad_column_wins" else V
    best = lg[:, :n].max(-1).values
    hit = lg[:, :n] == best[:, None]
    idx = torch.arange(n).expand_as(hit)
    ids = (torch.where(hit, idx, -1).max(-1).values if mut == "tie_high"
           else torch.where(hit, idx, n).min(-1).values)
    return lg[:, :V], best, ids


def book(state, vals, ids, max_steps, stop0, stop1):
    """The step's bookkeeping from each row's (best value, id): glue_ref.greedy_step on
    single-block partials.  -> the new state."""
    s, _ = glue_ref.greedy_step(state, vals.reshape(-1, 1).to(F32), ids.reshape(-1, 1).to(I32),
                                max_steps, stop0, stop1)
    return s


def step(m, tok, pos, kc, vc, dtype=F64, handoff=None, temperature=1.0):
    """One whole decode step by the definitions, in ``dtype``.  m: dict(wte, wpe, layers = 12
    dicts(ln1, attn_w, attn_b, proj_w, proj_b, ln2, fc_w, fc_b, mproj_w, mproj_b), lnf, head_w,
    head_b, V); ln1 / ln2 / lnf = (g, beta), or None where the affine is folded into the weights.
    kc / vc: 12 caches [>= R][12][Lmax][64].  ``handoff`` = bf16: round at exactly the kernel's
    hand-off points (the embedding sum in f32 and its bf16 copy, q / k / v, att, every xb, hid).
    -> dict(x [R, 768] after block 11, k / v: 12 x [R, 12, 64] written at pos, logits [R, V])."""
    R = tok.numel()
    rd = (lambda v: v) if handoff is None else (lambda v: _store(v, handoff))
    if handoff is None:
        x = m["wte"][tok.long()].to(dtype) + m["wpe"][pos.long()].to(dtype)
    else:
        x = embed_sum(m["wte"], m["wpe"], tok, pos).to(dtype)
    ks, vs = [], []
    for l, ly in enumerate(m["layers"]):
        q, kc2, vc2 = phase_a(rd(x), ly["attn_w"], ly["attn_b"], None, kc[l][:R], vc[l][:R], pos,
                              dtype, handoff, ln=ly["ln1"])
        ar = torch.arange(R)
        ks.append(kc2[ar, :, pos.long()])
        vs.append(vc2[ar, :, pos.long()])
        att = phase_b(q, kc2, vc2, pos, dtype, handoff)
        x = phase_ce(att, ly["proj_w"], ly["proj_b"], x, dtype)
        hid, _ = phase_d(rd(x), ly["fc_w"], ly["fc_b"], None, dtype, handoff, ln=ly["ln2"])
        x = phase_ce(hid, ly["mproj_w"], ly["mproj_b"], x, dtype)
    lg, best, ids = phase_f(rd(x), m["head_w"], m["head_b"], None, m["V"], temperature, dtype,
                            ln=m["lnf"])
    return dict(x=x, k=ks, v=vs, logits=lg, best=best, ids=ids)


# ------------------------------------------------------------------ the cases
V_SMALL = 9217               # 16 * 576 + 1: the last vocab block has one real column; >= 16 * 192 * 3
LAYER = 7                    # the isolated phases of "a layer > 0"
GRIDS = {"bf16": (48, 96, 192), "f32": (192,)}
RS = (1, 17, 64)
ROW_KINDS = (0, 16, 2, "eq")     # |mean| / std of row i: ROW_KINDS[(i + R) % 4]; "eq": all equal


def _gen(*parts):
    s = 0
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % 1000003
    g = torch.Generator()
    g.manual_seed(s)
    return g


def _st(mode):
    return BF16 if mode == "bf16" else F32


def _kstep(mode):
    """k per accumulation step of the float32 yardstick: one MFMA 16x16x32 of the bf16 kernels;
    the f32 kernels' v_mfma_f32_16x16x4_f32 is bitwise an fmaf chain, one k at a time."""
    return 32 if mode == "bf16" else 1


def fold(W, b, g, beta, st):
    """The host fold by its definition: W' = st(W diag(g)), b' = f32(b + W beta) summed in f64,
    cs = f32 of the f64 column sums of the ROUNDED W'; cs_u those of the unrounded W diag(g)."""
    Wu = W * g[None, :]
    Wp = Wu.to(st)
    return dict(w=Wp, b=(b.double() + W.double() @ beta.double()).float(),
                cs=Wp.double().sum(1).float(), cs_u=Wu.double().sum(1).float())


@functools.lru_cache(maxsize=None)
def layer_tables(mode):
    """One block's tables in the storage type of ``mode``, folded here from seeded f32 masters.
    c_fc's scale puts pre-activations beyond +-10 and next to 0 (test_grid_ref asserts it)."""
    g = _gen("layer")
    st = _st(mode)
    r = lambda *s: torch.randn(*s, generator=g)
    aff = lambda: (1.0 + 0.1 * r(D), 0.1 * r(D))
    a = fold(0.1 * r(QKVN, D), 0.02 * r(QKVN), *aff(), st)
    f = fold(0.15 * r(DFF, D), 0.02 * r(DFF), *aff(), st)
    return dict(attn=a, fc=f, proj_w=(0.05 * r(D, D)).to(st), proj_b=0.02 * r(D),
                mproj_w=(0.02 * r(D, DFF)).to(st), mproj_b=0.02 * r(D))


def ln_rows(R, mode, tag):
    """R LayerNorm input rows of std ~1 in the storage type: row i has |mean| / std of
    ROW_KINDS[(i + R) % 4], or every element equal ("eq": variance 0)."""
    g = _gen("rows", R, tag)
    x = torch.randn(R, D, generator=g)
    for i in range(R):
        kind = ROW_KINDS[(i + R) % 4]
        if kind == "eq":
            x[i] = 0.75 + 0.125 * (i % 3)
        else:
            x[i] = x[i] - x[i].mean() + kind * x[i].std(unbiased=False) * (1 if i % 2 else -1)
    return x.to(_st(mode))


def row_ratio(x):
    """|mean| / std of each row (float64; inf for an all-equal row that is not zero)."""
    x = x.double()
    return x.mean(-1).abs() / x.std(-1, unbiased=False)


def _positions(R, Lmax, g, must=()):
    pos = torch.randint(1, Lmax, (R,), generator=g, dtype=I32)
    must = [p for p in must][:R]
    pos[:len(must)] = torch.tensor(must, dtype=I32)
    return pos


def _cache(rows, Lmax, st):
    return torch.full((rows, NH, Lmax, HD), SENT, dtype=st)


@functools.lru_cache(maxsize=None)
def case_a(mode, layer, R):
    """Phase A of block ``layer`` (0: the embedding path; LAYER: rows from WS_XB) at R rows,
    Lmax 40, ragged pos.  Block 0's rows come out of crafted wte / wpe rows: the same row kinds,
    distinct tokens, the all-equal rows at positions of their own whose wpe row is all equal."""
    st, Lmax, V = _st(mode), 40, V_SMALL
    g = _gen("a", mode, layer, R)
    t = layer_tables(mode)["attn"]
    rows = ln_rows(R, mode, "a")
    c = dict(mode=mode, layer=layer, R=R, Lmax=Lmax, V=V, tab=t)
    eq = [i for i in range(R) if ROW_KINDS[(i + R) % 4] == "eq"]
    eq_pos = list(range(2, 2 + 2 * len(eq), 2))                 # even positions 2 .. 32
    free = [p for p in range(1, Lmax) if p not in eq_pos]
    pos = torch.tensor([free[int(j)] for j in torch.randint(0, len(free), (R,), generator=g)], dtype=I32)
    if R > 1:
        pos[0], pos[1] = 1, Lmax - 1
    for i, p in zip(eq, eq_pos):
        pos[i] = p
    tok = torch.randperm(V, generator=g)[:R].to(I32)
    tok[0] = V - 1
    c.update(pos=pos, tok=tok, kc=_cache(R + 1, Lmax, st), vc=_cache(R + 1, Lmax, st))
    if layer == 0:
        wte = (0.1 * torch.randn(V, D, generator=g)).to(st)
        wpe = (0.005 * torch.randn(Lmax, D, generator=g)).to(st)
        for i, p in zip(eq, eq_pos):
            wpe[p] = 0.125 + 0.03125 * (i % 4)
        wte[tok.long()] = (0.1 * rows.float()).to(st)
        c.update(wte=wte, wpe=wpe)
        e = embed_sum(wte, wpe, tok, pos)
        c["x"] = e.to(BF16) if mode == "bf16" else e
    else:
        c["x"] = rows
    cs = t["cs"] if mode == "bf16" else None
    out = {}
    for dt in (F64, F32):
        out[dt] = phase_a(c["x"], t["w"], t["b"], cs, c["kc"][:R], c["vc"][:R], pos, dt, None, _kstep(mode))
    c["ref"], c["yard"] = out[F64], out[F32]
    return c


def mutate_a(c, mut):
    t, R = c["tab"], c["R"]
    return phase_a(c["x"], t["w"], t["b"], t["cs"], c["kc"][:R], c["vc"][:R], c["pos"], F64,
                   None, mut=mut, cs_mut=t["cs_u"])


@functools.lru_cache(maxsize=None)
def case_d(mode, R):
    """Phase D of block LAYER at R rows: the row kinds of ln_rows."""
    st = _st(mode)
    t = layer_tables(mode)["fc"]
    c = dict(mode=mode, layer=LAYER, R=R, tab=t, x=ln_rows(R, mode, "d"))
    cs = t["cs"] if mode == "bf16" else None
    c["ref"], c["pre"] = phase_d(c["x"], t["w"], t["b"], cs, F64, None, _kstep(mode))
    c["yard"], _ = phase_d(c["x"], t["w"], t["b"], cs, F32, None, _kstep(mode))
    return c


def mutate_d(c, mut):
    t = c["tab"]
    return phase_d(c["x"], t["w"], t["b"], t["cs"], F64, None, mut=mut, cs_mut=t["cs_u"])[0]


B_POS = (1, 2, 31, 32, 33, 63, 64, 65, 99)
B_SPAN, B_ONE, B_NEW = (8, 3), (7, 5), (6, 7)     # (row, head): scores past +-40 (pos 99), one
                                                   # cached key dominates (pos 65), the new key (64)


@functools.lru_cache(maxsize=None)
def case_b(mode):
    """Phase B of block LAYER: R = 19, Lmax = 100, pos from 1 to Lmax - 1 across the chunk edges,
    q / K / V of std ~1; three (row, head) units with scores past +-40, one dominating cached key
    and a dominating new key.  Slots past pos hold the sentinel: a key read there shows."""
    st, R, Lmax = _st(mode), 19, 100
    g = _gen("b", mode)
    pos = _positions(R, Lmax, g, B_POS)
    q = torch.randn(R, D, generator=g)
    kc, vc = _cache(R + 1, Lmax, st), _cache(R + 1, Lmax, st)
    for r in range(R):
        p = int(pos[r])
        kc[r, :, :p + 1] = torch.randn(NH, p + 1, HD, generator=g).to(st)
        vc[r, :, :p + 1] = torch.randn(NH, p + 1, HD, generator=g).to(st)
    r, h = B_SPAN
    q[r, 64 * h:64 * h + 64] *= 40.0
    q = q.to(st)
    r, h = B_ONE
    kc[r, h, 40] = (4.0 * q[r, 64 * h:64 * h + 64].float()).to(st)
    r, h = B_NEW
    kc[r, h, int(pos[r])] = (4.0 * q[r, 64 * h:64 * h + 64].float()).to(st)
    c = dict(mode=mode, layer=LAYER, R=R, Lmax=Lmax, pos=pos, q=q, kc=kc, vc=vc)
    c["ref"] = phase_b(q, kc, vc, pos, F64, None)
    c["yard"] = phase_b(q, kc, vc, pos, F32, None)
    return c


def mutate_b(c, mut):
    return phase_b(c["q"], c["kc"], c["vc"], c["pos"], F64, None, mut=mut)


@functools.lru_cache(maxsize=None)
def case_ce(mode, which, layer, R):
    """Phase C (which = "C": a = att, K = 768; block 0: x_old is the embedding sum) or E (a = hid,
    K = 3072) of block ``layer`` at R rows."""
    st = _st(mode)
    g = _gen("ce", mode, which, layer, R)
    t = layer_tables(mode)
    w, b = (t["proj_w"], t["proj_b"]) if which == "C" else (t["mproj_w"], t["mproj_b"])
    K = w.shape[1]
    a = torch.randn(R, K, generator=g)
    if which == "E":
        a = act_apply(2.0 * a, "gelu_tanh")
    c = dict(mode=mode, which=which, layer=layer, R=R, w=w, b=b, a=a.to(st), Lmax=40, V=V_SMALL)
    c["pos"] = _positions(R, 40, g, (39, 1))
    c["tok"] = torch.randperm(V_SMALL, generator=g)[:R].to(I32)
    if which == "C" and layer == 0:
        c["wte"] = torch.randn(V_SMALL, D, generator=g).to(st)
        c["wpe"] = (0.5 * torch.randn(40, D, generator=g)).to(st)
        c["x_old"] = embed_sum(c["wte"], c["wpe"], c["tok"], c["pos"])
    else:
        c["x_old"] = 2.0 * torch.randn(R, D, generator=g)
    c["ref"] = phase_ce(c["a"], w, b, c["x_old"], F64, _kstep(mode))
    c["yard"] = phase_ce(c["a"], w, b, c["x_old"], F32, _kstep(mode))
    return c


def mutate_ce(c, mut):
    return phase_ce(c["a"], c["w"], c["b"], c["x_old"], F64, mut=mut)


# F: (row, the ids that share the row's largest logit exactly)
F_TIES = ((0, (V_SMALL - 1,)),                 # the single real column of the last block
          (1, (400, 401)),                     # one quad (one lane's 4 columns)
          (2, (1000, 1004)),                   # two lane groups of one block
          (3, (2000, 2000 + 16 * 48)),         # blocks b and b + G, G = 48 / 96 / 192
          (4, (3001, 3001 + 16 * 96)),
          (5, (100, 100 + 16 * 192)),
          (6, (5000, 5016)))                   # neighbouring blocks
F_VARIANTS = {"t1": dict(R=21, temperature=1.0, shift=0.0),
              "t07neg": dict(R=64, temperature=0.7, shift=-100.0)}


@functools.lru_cache(maxsize=None)
def case_f(mode, variant):
    """Phase F at V = 9217.  Rows 0 .. 7 own planted winners (F_TIES: duplicated table rows, so
    the tie is exact wherever the two columns are computed); "t07neg": temperature 0.7 and every
    logit of every row negative (a padded column's 0 would win if it were not masked)."""
    st, V = _st(mode), V_SMALL
    p = F_VARIANTS[variant]
    R, Vp = p["R"], 16 * (-(-V // 16))
    g = _gen("f", mode, variant)
    x = torch.randn(R, D, generator=g)
    x = (x + 2.0 * (torch.arange(R) % 2)[:, None]).to(st)
    w = torch.zeros(Vp, D)
    w[:V] = 0.1 * torch.randn(V, D, generator=g)
    b = torch.zeros(Vp)
    b[:V] = 0.5 * torch.randn(V, generator=g)
    mean, rstd = ln_stats(x, F64)
    y = ((x.double() - mean) * rstd).float()
    for r, ids in F_TIES:
        for v in ids:
            w[v] = 0.05 * y[r]
            b[v] = 0.25
    b[:V] += p["shift"]
    w = w.to(st)
    cs = w.double().sum(1).float() if mode == "bf16" else None
    c = dict(mode=mode, variant=variant, R=R, V=V, x=x, w=w, b=b, cs=cs, temperature=p["temperature"])
    c["ref"] = phase_f(x, w, b, cs, V, p["temperature"], F64, _kstep(mode))
    c["yard"] = phase_f(x, w, b, cs, V, p["temperature"], F32, _kstep(mode))
    return c


def mutate_f(c, mut):
    return phase_f(c["x"], c["w"], c["b"], c["cs"], c["V"], c["temperature"], F64, mut=mut)


def f_tolerance(c):
    """(yardstick, tolerance) of the logits: plain form (the key carries an f32 value)."""
    yard, tol = tolerance(c["ref"][0], c["yard"][0])
    return yard, float(tol.max())


def f_candidates(c):
    """Per row the ids whose reference logit lies within the tolerance of the row's maximum, and
    whether they are exactly the planted set (then the lowest of them is the answer) or a single
    id; otherwise either of the row's candidates is accepted."""
    lg, best, _ = c["ref"]
    _, tol = f_tolerance(c)
    planted = dict(F_TIES)
    out = []
    for r in range(c["R"]):
        cand = torch.nonzero(lg[r] >= best[r] - tol).reshape(-1).tolist()
        strict = len(cand) == 1 or (r in planted and tuple(cand) == tuple(sorted(planted[r])))
        out.append((cand, strict))
    return out


BOOK_CASES = {"mid": dict(step=2, max_steps=5), "last": dict(step=4, max_steps=5)}
BOOK_DONE = (2, 9, 20)       # rows already done at entry


def book_case(name):
    """The bookkeeping after F of case_f("bf16" / "f32", "t1"): rows already done, row 1 stopping
    on stop0 (its planted id 400), row 0 on stop1 (id 9216), and the last step."""
    p = BOOK_CASES[name]
    R = F_VARIANTS["t1"]["R"]
    g = _gen("book", name)
    done = torch.zeros(R, dtype=I32)
    done[list(BOOK_DONE)] = 1
    out_ids = torch.full((R, p["max_steps"]), -7, dtype=I32)
    out_ids[:, :p["step"]] = torch.randint(0, V_SMALL, (R, p["step"]), generator=g, dtype=I32)
    out_len = torch.full((R,), p["step"], dtype=I32)
    out_len[list(BOOK_DONE)] = 1
    state = dict(pos=_positions(R, 40, g, (1, 38)), done=done, out_len=out_len, out_ids=out_ids,
                 next_tok=torch.randint(0, V_SMALL, (R,), generator=g, dtype=I32),
                 step_ctr=torch.tensor([p["step"]], dtype=I32), all_done=torch.zeros(3, dtype=I32))
    return dict(state=state, max_steps=p["max_steps"], stop0=400, stop1=V_SMALL - 1, R=R)
